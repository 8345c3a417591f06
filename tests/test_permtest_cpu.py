"""CPU: the restatement of the paired permutation test (permtest_ref) on hand-computed SplitMix64 values and a worked example, the host
summaries (RetrievalMetrics.permutation_summary / ir_permutation_summary) on hand-made statistics -- the exact tie above all --, the
calibration of the test on the restatement, the host-side refusals of nr_permtest_rank_stats / nr_permtest_unit_sums, the evaluator's
argument checks and the command-line flags."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import permtest_ref as P
from neighborretr_amd import evaluator, hip
from neighborretr_amd.metrics import RetrievalMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = SimpleNamespace


# ---- the swap bits ----------------------------------------------------------------------------------------------------------------------
def test_splitmix64_and_swap_bits_check_values():
    # SplitMix64 seeded with 1234567: its first outputs (the published check values of the generator)
    assert [P.sm64(1234567, c) for c in range(3)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    # the salted stream of seed 42: SM64(42 ^ salt, (p << 32) | u), worked with Python's integers
    assert P.SALT == int.from_bytes(b"permtest", "big") == 0x7065726D74657374
    want = {(0, 0): 0x229FCCBEF9A44A86, (0, 1): 0x9C19B6188DCE9B50, (0, 2): 0x1ABB5C839E0160AB,
            (1, 0): 0x816340C0749955EE, (1, 1): 0x2EAB0C10EFD353E8, (1, 2): 0x0408772518524556}
    for (p, u), x in want.items():
        assert P.sm64(42 ^ P.SALT, (p << 32) | u) == x
        assert P.swap_bit(42, p, u) == x >> 63
    assert [P.swap_bits(42, p, 8) for p in range(3)] == [[0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 1, 1, 0, 1, 1], [0, 1, 0, 0, 1, 1, 0, 0]]
    # the vectorised form is the same function, whatever p0; the largest seed and a late permutation wrap modulo 2^64
    assert P.swap_matrix(42, 0, 3, 8).tolist() == [P.swap_bits(42, p, 8) for p in range(3)]
    assert P.swap_matrix(42, 2, 1, 8).tolist() == [P.swap_bits(42, 2, 8)]
    late = (1 << 31) - 3
    assert P.swap_matrix((1 << 64) - 2, late, 2, 70).tolist() == [P.swap_bits((1 << 64) - 2, late + i, 70) for i in range(2)]
    # the salt keeps the stream apart from the bootstrap's at equal seeds, and the bits are balanced
    assert [P.sm64(42, u) >> 63 for u in range(64)] != P.swap_bits(42, 0, 64)
    assert abs(P.swap_matrix(7, 0, 100, 1000).mean() - 0.5) < 0.005


# ranking a: unit 2 is empty, unit 1 holds a tie, one rank (70000) needs a second digit of the select; b has one entry per unit
RANKS_A, END_A = [0, 3, 3, 70000, 1, 0, 12], [0, 2, 2, 3, 6]
RANKS_B, END_B = [0, 0, 5, 2, 9], [0, 1, 2, 3, 4]


def test_worked_example():
    got = P.rank_stats(RANKS_A, END_A, RANKS_B, END_B, cuts=(1, 5, 10, 50), seed=42, p0=0, n_perm=3)
    assert got.dtype == np.int64 and got.shape == (3, 2, 8)
    # by hand, permutation 0 has the bits 0 1 0 0 0: X = a0 b1 a2 a3 a4 = {0} {0} {} {70000} {1, 0, 12}, Y = b0 a1 b2 b3 b4
    assert got[0].tolist() == [[6, 70013, 0, 1, 3, 4, 4, 5], [6, 22, 3, 3, 1, 4, 6, 6]]
    # permutation 1: bits 1 0 0 1 1: X = b0 a1 a2 b3 b4 = {0} {3, 3} {} {2} {9}
    assert got[1, 0].tolist() == [5, 17, 3, 3, 1, 4, 5, 5]
    for row in got:                                                            # the two sides hold every entry once
        assert (row[0] + row[1])[[0, 1, 4, 5, 6, 7]].tolist() == [12, 70035, 4, 8, 10, 11]
    assert np.array_equal(P.rank_stats(RANKS_A, END_A, RANKS_B, END_B, seed=42, p0=1, n_perm=2), got[1:])
    # swapping the rankings swaps the sides
    assert np.array_equal(P.rank_stats(RANKS_B, END_B, RANKS_A, END_A, seed=42, n_perm=3), got[:, ::-1])
    # single-entry units: the vectorised form is the restatement
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 60, 37), rng.integers(0, 2000, 37)
    assert np.array_equal(P.single_entry_stats(a, b, (1, 10), seed=9, p0=2, n_perm=6),
                          P.rank_stats(a, np.arange(37), b, np.arange(37), (1, 10), seed=9, p0=2, n_perm=6))


def test_unit_sums_worked_example():
    va = np.asarray([[1, 10], [1, -20], [0, 0], [1, 1 << 40]], dtype=np.int64)
    vb = np.asarray([[1, 7], [0, 0], [1, 5], [1, -(1 << 41)]], dtype=np.int64)
    got = P.unit_sums(va, vb, seed=42, n_perm=2)                               # bits 0 1 0 0 and 1 0 0 1
    assert got.tolist() == [[2, 10 + 0 + 0 + (1 << 40)], [3, 7 - 20 + 0 - (1 << 41)]]
    ones = np.ones((8, 1), dtype=np.int64)
    assert P.unit_sums(0 * ones, ones, seed=42, n_perm=3)[:, 0].tolist() == [sum(P.swap_bits(42, p, 8)) for p in range(3)]


# ---- the summaries on hand-made statistics ----------------------------------------------------------------------------------------------
def test_the_exact_tie_counts_as_a_tie():
    """Observed (ha, hb, n) = (1, 0, 3).  The relabellings (hx, hy, n) = (2, 1, 3) and (3, 2, 3) have the same difference of R@1, one
    third; with the summaries' own fp64 formula 100 h / n the second one does not compare equal: the comparison is made on
    cross-multiplied integers."""
    assert 100 * 3 / 3 - 100 * 2 / 3 != 100 * 1 / 3 - 100 * 0 / 3
    #                  n  sum lo hi <1      n  sum lo hi <1
    stats = np.asarray([[[3, 0, 0, 0, 2], [3, 0, 0, 0, 1]],                     # (2, 1, 3): tied with the observed
                        [[3, 0, 0, 0, 3], [3, 0, 0, 0, 2]],                     # (3, 2, 3): tied, and not in fp64
                        [[3, 0, 0, 0, 0], [3, 0, 0, 0, 1]],                     # (0, 1, 3): the mirror image, tied in |d| only
                        [[3, 0, 0, 0, 1], [3, 0, 0, 0, 1]]])                    # (1, 1, 3): d = 0
    for summary in (RetrievalMetrics.permutation_summary, P.permutation_summary):
        s = summary(stats, (1,), [0, 5, 5], [5, 5, 5])
        assert (s["n_perm"], s["n_empty"], s["kept"]) == (4, 0, 4)
        assert s["R1"]["diff"] == pytest.approx(100 / 3, rel=1e-15)
        assert s["R1"]["p_two"] == (1 + 3) / 5 and s["R1"]["p_ge"] == (1 + 2) / 5 and s["R1"]["p_le"] == 1.0
        only = summary(stats[:1], (1,), [0, 5, 5], [5, 5, 5])["R1"]             # the case of the definition alone
        assert (only["p_two"], only["p_ge"], only["p_le"]) == (1.0, 1.0, 1.0)


def test_permutation_summary_by_hand():
    #                    n  sum lo hi <1 <5
    stats = np.asarray([[[4, 10, 1, 3, 1, 3], [2, 4, 2, 2, 0, 2]],             # R1 25 - 0, MeanR 2.5 - 2, MedianR mid 3 - 3, low 2 - 3
                        [[0, 0, -1, -1, 0, 0], [6, 14, 1, 2, 1, 5]],           # X is empty: dropped
                        [[5, 5, 0, 1, 3, 5], [1, 9, 9, 9, 0, 0]],              # R1 60 - 0, MeanR 1 - 9, MedianR mid 1.5 - 10, low 1 - 10
                        [[3, 7, 2, 2, 0, 2], [3, 7, 0, 5, 1, 2]]])             # R1 0 - 33.3, MeanR equal, MedianR mid 3 - 3.5, low 3 - 1
    a, b = [0, 0, 3, 7], [2, 9]                                                # observed: R1 50 - 0, R5 75 - 50, MeanR 3.5 - 6.5, MedianR 2.5 - 6.5
    for summary in (RetrievalMetrics.permutation_summary, P.permutation_summary):
        s = summary(stats, (1, 5), a, b, "mid", seed=9)
        assert {k: s[k] for k in ("n_perm", "n_empty", "kept", "seed", "median")} == dict(n_perm=4, n_empty=1, kept=3, seed=9, median="mid")
        assert set(s) == {"n_perm", "n_empty", "kept", "seed", "median", "R1", "R5", "MedianR", "MeanR"}
        assert s["R1"] == dict(diff=50.0, p_two=2 / 4, p_ge=2 / 4, p_le=3 / 4)                 # d_p: 25, 60, -33.3
        assert s["MeanR"] == dict(diff=-3.0, p_two=2 / 4, p_ge=3 / 4, p_le=2 / 4)              # d_p: 0.5, -8, 0
        assert s["MedianR"] == dict(diff=-4.0, p_two=2 / 4, p_ge=3 / 4, p_le=2 / 4)            # d_p: 0, -8.5, -0.5
        low = summary(stats, (1, 5), a, b, "low")
        assert low["MedianR"] == dict(diff=-2.0, p_two=3 / 4, p_ge=3 / 4, p_le=2 / 4)          # observed 1 - 3; d_p: -1, -9, 2
        assert low["R1"] == s["R1"] and low["median"] == "low"
    none = RetrievalMetrics.permutation_summary(stats[1:2], (1, 5), a, b)
    assert (none["n_empty"], none["kept"]) == (1, 0) and none["R1"]["p_two"] == 1.0            # (1 + 0) / (1 + 0)
    assert np.isnan(RetrievalMetrics.permutation_summary(stats, (1, 5), a, [])["R1"]["p_two"])  # an empty ranking: no figure
    with pytest.raises(ValueError, match="median"):
        RetrievalMetrics.permutation_summary(stats, (1, 5), a, b, "high")
    with pytest.raises(ValueError, match="stats"):
        RetrievalMetrics.permutation_summary(stats, (1,), a, b)
    with pytest.raises(ValueError, match="stats"):
        RetrievalMetrics.permutation_summary(stats[:, 0], (1, 5), a, b)


def _random_pair(rng, U, high=60):
    sa, sb = rng.integers(0, 4, U), rng.integers(0, 4, U)
    return (rng.integers(0, high, int(sa.sum())), np.cumsum(sa) - 1), (rng.integers(0, high, int(sb.sum())), np.cumsum(sb) - 1)


def test_summary_equals_the_restatement_and_its_symmetries():
    rng = np.random.default_rng(1)
    a, b = _random_pair(rng, 50)
    stats = P.rank_stats(*a, *b, seed=3, n_perm=300)
    for median in ("mid", "low"):
        got = RetrievalMetrics.permutation_summary(torch.from_numpy(stats), P.DEFAULT_CUTS, a[0], b[0], median, seed=3)
        assert got == P.permutation_summary(stats, P.DEFAULT_CUTS, a[0], b[0], median, seed=3)
    # a ranking against itself: diff 0 and every p = 1
    same = RetrievalMetrics.permutation_summary(P.rank_stats(*a, *a, seed=3, n_perm=100), P.DEFAULT_CUTS, a[0], a[0])
    for name in ("R1", "R5", "R10", "R50", "MedianR", "MeanR"):
        assert same[name] == dict(diff=0.0, p_two=1.0, p_ge=1.0, p_le=1.0), name
    # swapping A and B swaps the sides: diff negated, p_ge and p_le exchanged, p_two kept
    ab = RetrievalMetrics.permutation_summary(stats, P.DEFAULT_CUTS, a[0], b[0], seed=3)
    ba = RetrievalMetrics.permutation_summary(P.rank_stats(*b, *a, seed=3, n_perm=300), P.DEFAULT_CUTS, b[0], a[0], seed=3)
    assert any(ab[name]["p_ge"] != ab[name]["p_le"] for name in ("R1", "R5", "MeanR"))
    for name in ("R1", "R5", "R10", "R50", "MedianR", "MeanR"):
        assert ba[name] == dict(diff=-ab[name]["diff"], p_two=ab[name]["p_two"], p_ge=ab[name]["p_le"], p_le=ab[name]["p_ge"]), name


def test_ir_summary_equals_the_restatement_and_its_symmetries():
    rng = np.random.default_rng(2)
    one = RetrievalMetrics.IR_FIXED_ONE
    ca, cb = (np.concatenate([rng.integers(0, 3, (40, 1)), rng.integers(0, one, (40, 4))], axis=1).astype(np.int64) for _ in range(2))
    ca[:, 1:] *= ca[:, :1]                                                      # a unit's sums are at most its count
    cb[:, 1:] *= cb[:, :1]
    sums = P.unit_sums(ca, cb, seed=5, n_perm=200)
    got = RetrievalMetrics.ir_permutation_summary(torch.from_numpy(sums), ca, cb, seed=5)
    assert got == P.ir_permutation_summary(sums, ca, cb, seed=5)
    assert set(got) == {"n_perm", "n_empty", "kept", "seed", "MRR", "mAP", "nDCG10", "RPrec"} and got["kept"] == 200
    point = RetrievalMetrics._ir_values(ca.sum(0, keepdims=True))[0]["MRR"][0] - RetrievalMetrics._ir_values(cb.sum(0, keepdims=True))[0]["MRR"][0]
    assert got["MRR"]["diff"] == pytest.approx(point, rel=1e-12)
    same = RetrievalMetrics.ir_permutation_summary(P.unit_sums(ca, ca, seed=5, n_perm=50), ca, ca)
    ba = RetrievalMetrics.ir_permutation_summary(P.unit_sums(cb, ca, seed=5, n_perm=200), cb, ca, seed=5)
    for name in RetrievalMetrics.IR_METRICS:
        assert same[name] == dict(diff=0.0, p_two=1.0, p_ge=1.0, p_le=1.0)
        assert ba[name] == dict(diff=-got[name]["diff"], p_two=got[name]["p_two"], p_ge=got[name]["p_le"], p_le=got[name]["p_ge"])
    # a side without a query is dropped: one unit carries every query of b, a has none
    lone_a, lone_b = np.zeros((3, 5), dtype=np.int64), np.zeros((3, 5), dtype=np.int64)
    lone_b[1] = [2, 2 * one, 2 * one, 2 * one, 2 * one]
    lone_a[1] = [1, one // 2, one // 2, 0, 0]
    s = RetrievalMetrics.ir_permutation_summary(P.unit_sums(lone_a, lone_b, seed=1, n_perm=20), lone_a, lone_b)
    assert s == P.ir_permutation_summary(P.unit_sums(lone_a, lone_b, seed=1, n_perm=20), lone_a, lone_b)
    assert s["n_empty"] == 0 and s["MRR"]["diff"] == -50.0                       # unit 1 is on both sides, whichever way it is swapped
    with pytest.raises(ValueError, match="sums"):
        RetrievalMetrics.ir_permutation_summary(sums[:, :4], ca, cb)
    with pytest.raises(ValueError, match="columns"):
        RetrievalMetrics.ir_permutation_summary(sums, ca, cb[:-1])


def test_format_permutation():
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 30, 40), rng.integers(0, 60, 40)
    s = RetrievalMetrics.permutation_summary(P.single_entry_stats(a, b, seed=1, n_perm=50), P.DEFAULT_CUTS, a, b, seed=1)
    line = RetrievalMetrics.format_permutation(s, prefix="text->video [DSL b=20] - raw ")
    assert line.startswith("text->video [DSL b=20] - raw R@1: ") and line.endswith("(paired permutation test vs raw, 50 permutations)")
    assert line.count(" p=") == 5 and "Median R: " in line and f"Mean R: {s['MeanR']['diff']:+.2f} p={s['MeanR']['p_two']:.4f}" in line
    s["n_empty"] = 2
    assert RetrievalMetrics.format_permutation(s, versus="compared").endswith("(paired permutation test vs compared, 50 permutations, 2 empty)")
    ir = {"n_perm": 9, "n_empty": 0, "kept": 9, "seed": 0, **{n: dict(diff=1.5, p_two=0.25, p_ge=0.2, p_le=0.9) for n in RetrievalMetrics.IR_METRICS}}
    assert RetrievalMetrics.format_permutation(ir, "x ") == ("x MRR: +1.50 p=0.2500 - mAP: +1.50 p=0.2500 - nDCG@10: +1.50 p=0.2500 - "
                                                             "R-Prec: +1.50 p=0.2500 (paired permutation test vs raw, 9 permutations)")
    RetrievalMetrics(logger=None).log_permutation(s)                            # silent without a logger


# ---- the definition itself: the test holds its level and has power ----------------------------------------------------------------------
def test_calibration_of_the_randomisation_test():
    """Null: 200 data sets of U = 400 independent pairs of Bernoulli(0.4) hits (rank 0, else 7), 1000 permutations each: R@1's
    p_two <= 0.05 in at most 19 of them, 0.05 x 200 + 3 binomial standard deviations (3 sqrt(200 x .05 x .95) = 9.2); the restatement
    with these seeds gives 11.  Power: hit rates 0.60 against 0.40, 50 data sets: p_two <= 0.05 in at least 45; it gives 50."""
    U, n_perm = 400, 1000

    def rejections(trials, pa, pb, data_seed, perm_seed):
        count = 0
        for s in range(trials):
            rng = np.random.default_rng(data_seed + s)
            a, b = np.where(rng.random(U) < pa, 0, 7), np.where(rng.random(U) < pb, 0, 7)
            stats = P.single_entry_stats(a, b, (1,), seed=perm_seed + s, n_perm=n_perm)
            count += P.permutation_summary(stats, (1,), a, b, seed=perm_seed + s)["R1"]["p_two"] <= 0.05
        return count
    null, power = rejections(200, 0.4, 0.4, 0, 1000), rejections(50, 0.6, 0.4, 5000, 7000)
    print(f"null: {null} of 200 rejected at 0.05; power: {power} of 50")
    assert null <= 19
    assert power >= 45


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def _declaration(header, name):
    """(the comment in front of `name`'s declaration, its parameter list) from the header's text."""
    at = header.index(f"int {name}(")
    comment = header[header.rindex("/*", 0, at):at]
    return comment, header[at:header.index(");", at)]


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    comment, decl = _declaration(header, "nr_permtest_rank_stats")
    for word in ("SplitMix64", "0x7065726D74657374", ">> 63", "unit_end", "med_lo", "(n-1)/2", "NR_EINVAL", "2^24", "2^31 - 1", "NR_OK",
                 "HOST", "side X", "E_a + E_b"):
        assert word in comment, word
    args, res = hip._SIGNATURES["nr_permtest_rank_stats"]
    assert len(args) == decl.count(",") + 1 == 14 and args[9] is ctypes.c_uint64 and res is ctypes.c_int
    assert [a is ctypes.c_void_p for a in args] == [bool(re.search(r"\*", part)) for part in decl.split(",")]
    comment, decl = _declaration(header, "nr_permtest_unit_sums")
    for word in ("values_a", "total_a + total_b - X", "2^62", "[1, 16]", "NR_EINVAL", "NR_OK", "nr_permtest_rank_stats"):
        assert word in comment, word
    args, res = hip._SIGNATURES["nr_permtest_unit_sums"]
    assert len(args) == decl.count(",") + 1 == 9 and args[4] is ctypes.c_uint64 and res is ctypes.c_int
    assert [a is ctypes.c_void_p for a in args] == [bool(re.search(r"\*", part)) for part in decl.split(",")]
    for name in ("nr_permtest_rank_stats", "nr_permtest_unit_sums"):
        assert name in hip.exported_symbols() and hasattr(hip.lib(), name)
    assert hip.PERM_SALT == P.SALT and (hip.BOOT_MAX_UNITS, hip.BOOT_MAX_CUTS, hip.BOOT_MAX_COLS) == (1 << 24, 8, 16)


def _caller(fn, names, good):
    def call(**over):
        a = list(good)
        for k, v in over.items():
            a[names.index(k)] = v
        return fn(*a)
    return call


def test_rank_stats_refuses_bad_arguments_before_any_launch():
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    cuts = (ctypes.c_int32 * 8)(1, 5, 10, 50, 60, 70, 80, 90)
    names = ("ranks_a", "end_a", "E_a", "ranks_b", "end_b", "E_b", "U", "cuts", "K", "seed", "p0", "n_perm", "out", "stream")
    call = _caller(hip.lib().nr_permtest_rank_stats, names, [p, p, 4, p, p, 4, 3, cuts, 4, 42, 0, 5, p, None])    # no device needed
    for name in ("ranks_a", "end_a", "ranks_b", "end_b", "cuts", "out"):            # a null pointer: both rankings are required
        assert call(**{name: None}) == EINVAL, name
    for U in (0, -1, (1 << 24) + 1):
        assert call(U=U) == EINVAL, U
    for K in (0, -1, 9):
        assert call(K=K) == EINVAL, K
    assert call(E_a=-1) == EINVAL and call(E_b=-1) == EINVAL
    assert call(p0=-1) == EINVAL and call(n_perm=-1) == EINVAL
    assert call(p0=(1 << 31) - 5, n_perm=5) == EINVAL and call(p0=(1 << 31) - 1, n_perm=1) == EINVAL
    for bad in ((0, 5, 10, 50), (1, 5, 5, 50), (5, 1, 10, 50), (-1, 5, 10, 50)):     # cut-offs: positive and strictly increasing
        assert call(cuts=(ctypes.c_int32 * 4)(*bad)) == EINVAL, bad
    # nothing to do: NR_OK without a launch, and the arguments are checked even then
    assert call(n_perm=0) == 0 and call(n_perm=0, p0=(1 << 31) - 1) == 0
    assert call(n_perm=0, U=1 << 24, K=8) == 0 and call(n_perm=0, U=1, K=1, E_a=0, E_b=0) == 0
    assert call(n_perm=0, K=4, cuts=(ctypes.c_int32 * 4)(0, 5, 10, 50)) == EINVAL and call(n_perm=0, ranks_b=None) == EINVAL


def test_unit_sums_refuses_bad_arguments_before_any_launch():
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    names = ("values_a", "values_b", "U", "Q", "seed", "p0", "n_perm", "out", "stream")
    call = _caller(hip.lib().nr_permtest_unit_sums, names, [p, p, 3, 5, 42, 0, 5, p, None])
    for name in ("values_a", "values_b", "out"):
        assert call(**{name: None}) == EINVAL, name
    for U in (0, -1, (1 << 24) + 1):
        assert call(U=U) == EINVAL, U
    for Q in (0, -1, 17):
        assert call(Q=Q) == EINVAL, Q
    assert call(p0=-1) == EINVAL and call(n_perm=-1) == EINVAL
    assert call(p0=(1 << 31) - 5, n_perm=5) == EINVAL and call(p0=(1 << 31) - 1, n_perm=1) == EINVAL
    assert call(n_perm=0) == 0 and call(n_perm=0, p0=(1 << 31) - 1, U=1 << 24, Q=16) == 0 and call(n_perm=0, Q=1, U=1) == 0
    assert call(n_perm=0, Q=17) == EINVAL and call(n_perm=0, values_b=None) == EINVAL


# ---- the evaluator's checks --------------------------------------------------------------------------------------------------------------
def test_evaluator_checks_the_permutation_arguments():
    assert evaluator._check_permutation(0) is None and evaluator._check_permutation(0, 5) is None
    assert evaluator._check_permutation(200, 3) == (200, 3) and evaluator._check_permutation(1 << 20) == (1 << 20, 0)
    for bad in (-1, (1 << 20) + 1, 2.5, "10", None, True):
        with pytest.raises(ValueError, match="permutation must"):
            evaluator._check_permutation(bad)
    for bad in (-1, (1 << 64) - 1, 0.5, None, True):
        with pytest.raises(ValueError, match="permutation_seed"):
            evaluator._check_permutation(10, bad)
    z = torch.zeros((4, 2, 8))
    for fn, extra in ((evaluator.sharded_metrics, ()), (evaluator.sharded_multi_sentence_metrics, ([0, 1, 2, 3],)),
                      (evaluator.sharded_metrics_with_hubness, (5,)), (evaluator.sharded_metrics_with_test_norm, ("is",)),
                      (evaluator.sharded_metrics_with_local_scaling, ("csls",)),
                      (evaluator.sharded_metrics_with_mutual_proximity, ("emp",))):
        head = (None, z, z, z[..., 0], z[..., 0])
        pos = head + extra + (None,) if fn is evaluator.sharded_multi_sentence_metrics else head + (None,) + extra
        with pytest.raises(ValueError, match="permutation must"):               # before any scoring: there is no model
            fn(*pos, permutation=-3)
        with pytest.raises(ValueError, match="permutation_seed"):
            fn(*pos, permutation=10, permutation_seed=-1)
    with pytest.raises(ValueError, match="permutation must"):
        evaluator.sharded_evaluation(None, z, z, z[..., 0], z[..., 0], None, permutation=1.5)


def test_flags_reach_the_driver_and_bad_values_are_refused_before_any_work():
    from neighborretr_amd import training
    c, kw = evaluator.correction_from_args(NS(test_norm="dsl", permutation=200, permutation_seed=7), None)
    assert c.key == "test_norm" and (kw["permutation"], kw["permutation_seed"]) == (200, 7)
    _, kw = evaluator.correction_from_args(NS(permutation=50, compare_model="other.bin"), None)
    assert (kw["permutation"], kw["permutation_seed"]) == (50, 0)
    for args in (NS(test_norm="dsl"), NS(test_norm="dsl", permutation=0, permutation_seed=9), NS(permutation=None)):
        assert "permutation" not in evaluator.correction_from_args(args, None)[1]   # off: the driver's arguments are today's
    for eval_epoch in (lambda a: training.eval_epoch(a, None, None, "cpu"), lambda a: _main().eval_epoch(a, None, None)):
        for bad in (-1, (1 << 20) + 1, 2.5, "many"):                              # no model, no data: nothing may be touched
            with pytest.raises(ValueError, match="permutation must"):
                eval_epoch(NS(test_norm="dsl", permutation=bad))
        for bad in (-4, (1 << 64) - 1, 0.5):
            with pytest.raises(ValueError, match="permutation_seed"):
                eval_epoch(NS(test_norm="dsl", permutation=100, permutation_seed=bad))
        with pytest.raises(ValueError, match="permutation needs a correction .* or compare_model"):
            eval_epoch(NS(permutation=100))
        with pytest.raises(ValueError, match="permutation needs a correction"):
            eval_epoch(NS(permutation=100, test_norm="none", compare_model=None, bootstrap=10))


def test_compare_evaluations_checks_its_arguments_before_any_launch():
    units = dict(entries=np.arange(3), unit_end=np.arange(3), median="mid")
    a = ({"units": units}, {"units": units})
    with pytest.raises(ValueError, match="permutation > 0"):
        evaluator.compare_evaluations(a, a, 0)
    with pytest.raises(ValueError, match="permutation must"):
        evaluator.compare_evaluations(a, a, -1)
    with pytest.raises(ValueError, match="permutation_seed"):
        evaluator.compare_evaluations(a, a, 10, permutation_seed=-1)
    with pytest.raises(ValueError, match="bootstrap_level"):
        evaluator.compare_evaluations(a, a, 10, bootstrap=5, bootstrap_level=1.0)
    with pytest.raises(ValueError, match="carries no units"):
        evaluator.compare_evaluations(a, ({}, {}), 10)
    other = dict(entries=np.arange(4), unit_end=np.arange(4), median="mid")
    with pytest.raises(ValueError, match="3 and 4 units"):
        evaluator.compare_evaluations(a, ({"units": other}, {"units": other}), 10)
    low = dict(units, median="low")
    with pytest.raises(ValueError, match="different medians"):
        evaluator.compare_evaluations(a, ({"units": low}, {"units": low}), 10)
    ir = ({"units": units, "ir": {"columns": np.zeros((3, 5), dtype=np.int64)}},) * 2
    short = ({"units": units, "ir": {"columns": np.zeros((3, 4), dtype=np.int64)}},) * 2
    with pytest.raises(ValueError, match="IR columns are \\(3, 5\\) and \\(3, 4\\)"):
        evaluator.compare_evaluations(ir, short, 10)
    with pytest.raises(ValueError, match="carries no columns"):
        evaluator.compare_evaluations(ir, ({"units": units, "ir": {}},) * 2, 10)
    nested = ({"units": units, "test_norm": {"units": units}},) * 2             # a correction both carry is compared too
    with pytest.raises(ValueError, match="3 and 4 units"):
        evaluator.compare_evaluations(nested, ({"units": units, "test_norm": {"units": other}},) * 2, 10)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _main():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main_retrieval
    return main_retrieval


def _parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
    return _main().get_args()


def test_main_retrieval_accepts_the_permutation_flags(monkeypatch, capsys):
    a = _parse([], monkeypatch)
    assert (a.permutation, a.permutation_seed, a.compare_model) == (0, 0, None)
    a = _parse(["--permutation", "200", "--permutation_seed", "7", "--test_norm", "dsl"], monkeypatch)
    assert (a.permutation, a.permutation_seed, a.test_norm) == (200, 7, "dsl")
    a = _parse(["--do_eval", "1", "--permutation", "64", "--compare_model", "other.bin"], monkeypatch)
    assert (a.permutation, a.compare_model) == (64, "other.bin")
    for argv, word in ((["--permutation", "-1", "--test_norm", "dsl"], "--permutation must"),
                       (["--permutation", str((1 << 20) + 1), "--test_norm", "dsl"], "--permutation must"),
                       (["--permutation", "10", "--permutation_seed", "-1", "--test_norm", "dsl"], "--permutation_seed"),
                       (["--permutation", "10"], "--permutation needs a correction"),
                       (["--do_eval", "1", "--compare_model", "other.bin"], "--compare_model"),
                       (["--permutation", "10", "--compare_model", "other.bin"], "--compare_model"),
                       (["--do_train", "1", "--do_eval", "1", "--permutation", "10", "--compare_model", "other.bin"], "--compare_model")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            _parse(argv, monkeypatch)
        assert word in capsys.readouterr().err
