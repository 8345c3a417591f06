"""CPU: the restatement of the paired permutation test of hubness (hubperm_ref) against hubness_from_occurrences, its own identities and
permtest_ref's swap bits; the host summary (RetrievalMetrics.hubness_moments / hubness_permutation_summary) on hand-made statistics --
the exact tie above all -- and against the restatement; the calibration of the test on the restatement; the host-side refusals of
nr_permtest_hubness; the evaluator's argument checks and the command-line flag."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hubperm_ref as H
import permtest_ref as P
from neighborretr_amd import evaluator, hip
from neighborretr_amd.metrics import RetrievalMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = SimpleNamespace
FIGURES = ("skewness", "anti_hub_pct", "hub_pct", "bad_hub_pct", "hub_occurrence_pct", "good_occurrence_pct", "max_occurrence")


def _lists(rng, n_lists, k, G, weight):
    """Top-k lists of popularity + noise, some slots absent, some indices outside the gallery."""
    pop = np.linspace(2.0, 0.0, G)
    idx = np.argsort(-(weight * pop[None, :] + rng.standard_normal((n_lists, G))), axis=1, kind="stable")[:, :k].astype(np.int32)
    if idx.shape[1] < k:
        idx = np.concatenate([idx, np.full((n_lists, k - idx.shape[1]), -1, dtype=np.int32)], axis=1)
    idx[rng.random(idx.shape) < 0.05] = -1
    idx[rng.random(idx.shape) < 0.02] = G + 3
    return idx


# ---- the restatement checks itself ----------------------------------------------------------------------------------------------------
def test_swap_bits_are_those_of_the_permutation_tests():
    assert H.SALT == P.SALT and H.GOLDEN == P.GOLDEN
    for seed, p in ((0, 0), (42, 1), ((1 << 64) - 2, (1 << 31) - 2)):
        assert [H.swap_bit(seed, p, u) for u in range(70)] == P.swap_bits(seed, p, 70)
        assert H.swap_matrix(seed, p, 1, 70).astype(np.int64).tolist() == [P.swap_bits(seed, p, 70)]
    assert np.array_equal(H.swap_matrix(7, 3, 5, 33).astype(np.int64), P.swap_matrix(7, 3, 5, 33))


def test_figures_on_unpermuted_counts_are_those_of_hubness_from_occurrences():
    """The six rational figures exactly; skewness to 1e-12 relative: two fp64 evaluations of one exact quantity."""
    rng = np.random.default_rng(0)
    for G, n_lists, k, weight in ((50, 80, 5, 2.0), (200, 200, 15, 0.5), (7, 3, 3, 0.0), (1000, 300, 10, 4.0)):
        idx = _lists(rng, n_lists, k, G, weight)
        gt = rng.integers(0, G, n_lists)
        N, GN = H.counts(idx.tolist(), G, gt, gt + 2)
        m = H.moments(N, GN)
        want = RetrievalMetrics.hubness_from_occurrences(N, GN, k, n_lists)
        got = H.figures(m, G)
        for name in H.RATIONAL:
            assert got[name] == want[name], name
        assert got["skewness"] == pytest.approx(want["skewness"], rel=1e-12, abs=0)
        assert RetrievalMetrics.hubness_moments(N, GN).tolist() == m             # the product's nine integers are the restatement's
    # a flat count has no spread: a = 0 and skewness 0.0, as hubness_from_occurrences says
    flat = H.moments([3] * 8, [1] * 8)
    assert H.skewness(flat, 8) == 0.0 == RetrievalMetrics.hubness_from_occurrences([3] * 8, [1] * 8, 3, 8)["skewness"]
    assert H.figures(flat, 8)["hub_pct"] == 0.0 and flat == [24, 72, 216, 0, 0, 0, 0, 8, 3]


def test_moments_by_hand():
    # G = 5, S1 = 10, mean 2: hubs are the items with 5 N > 20, N > 4
    N, GN = [6, 0, 3, 0, 1], [1, 0, 3, 0, 0]
    assert H.moments(N, GN) == [10, 46, 244, 2, 1, 6, 1, 4, 6]
    assert RetrievalMetrics.hubness_moments(N, GN).tolist() == [10, 46, 244, 2, 1, 6, 1, 4, 6]
    assert H.moments([5, 5, 0, 0, 0], [3, 2, 0, 0, 0]) == [10, 50, 250, 3, 2, 10, 1, 5, 5]      # N - GN > GN: 2 > 3 no, 3 > 2 yes
    assert H.moments([5, 5, 0, 0, 0], [3, 3, 0, 0, 0])[6] == 0 and H.moments([5, 5, 0, 0, 0], [2, 2, 0, 0, 0])[6] == 2
    with pytest.raises(ValueError):
        RetrievalMetrics.hubness_moments([1, 2], [1])


def test_sides_sum_to_the_rankings_and_identical_rankings_change_nothing():
    rng = np.random.default_rng(1)
    G, k = 30, 4
    sizes = rng.integers(0, 4, 12)                                               # 12 units, some empty
    n_lists = int(sizes.sum())
    unit_end = np.cumsum(sizes) - 1
    a, b = _lists(rng, n_lists, k, G, 2.0), _lists(rng, n_lists, k, G, 0.0)
    gt = rng.integers(0, G, n_lists)
    stats = H.hubness_stats(a, b, unit_end, G, gt, gt + 3, seed=5, n_perm=20)
    ma, mb = H.moments(*H.counts(a.tolist(), G, gt, gt + 3)), H.moments(*H.counts(b.tolist(), G, gt, gt + 3))
    assert stats.dtype == np.int64 and stats.shape == (20, 2, 9)
    for row in stats:
        assert row[0, 0] + row[1, 0] == ma[0] + mb[0] and row[0, 7] + row[1, 7] == ma[7] + mb[7]
    assert len({tuple(r[0]) for r in stats.tolist()}) > 1
    assert np.array_equal(H.hubness_stats(a, b, unit_end, G, gt, gt + 3, seed=5, p0=7, n_perm=5), stats[7:12])
    # swapping the rankings swaps the sides
    assert np.array_equal(H.hubness_stats(b, a, unit_end, G, gt, gt + 3, seed=5, n_perm=20), stats[:, ::-1])
    # A against itself: every side holds A's integers, every difference is 0 and every p is 1
    same = H.hubness_stats(a, a, unit_end, G, gt, gt + 3, seed=5, n_perm=20)
    assert all(side == ma for row in same.tolist() for side in row)
    for summary in (H.summary, RetrievalMetrics.hubness_permutation_summary):
        s = summary(same, ma, ma, G, 5)
        for name in FIGURES:
            assert s[name] == dict(diff=0.0, p_two=1.0, p_ge=1.0, p_le=1.0), name
    # the vectorised form of the calibration is the same function
    U = 9
    a1 = np.stack([rng.permutation(G)[:k] for _ in range(U)])
    b1 = np.stack([rng.permutation(G)[:k] for _ in range(U)])
    want = H.hubness_stats(a1, b1, np.arange(U), G, np.arange(U), np.arange(U) + 1, seed=11, p0=3, n_perm=12)
    assert np.array_equal(H.single_list_stats(a1, b1, G, seed=11, p0=3, n_perm=12), want)


# ---- the summary on hand-made statistics ---------------------------------------------------------------------------------------------
def _row(S1=6, S2=14, S3=36, anti=0, hubs=0, hub_occ=0, bad=0, good=0, mx=3):
    return [S1, S2, S3, anti, hubs, hub_occ, bad, good, mx]


def test_the_exact_tie_counts_as_a_tie():
    """G = 3.  Observed anti-hubs (A, B) = (1, 0).  The relabellings (2, 1) and (3, 2) have the same difference of anti_hub_pct, one
    third of 100; with the fp64 formula 100 anti / G the second one does not compare equal: the comparison is made on cross-multiplied
    integers."""
    assert 100 * 3 / 3 - 100 * 2 / 3 != 100 * 1 / 3 - 100 * 0 / 3
    stats = np.asarray([[_row(anti=2), _row(anti=1)],                            # tied with the observed
                        [_row(anti=3), _row(anti=2)],                            # tied, and not in fp64
                        [_row(anti=0), _row(anti=1)],                            # the mirror image: tied in |d| only
                        [_row(anti=1), _row(anti=1)]])                           # d = 0
    for summary in (RetrievalMetrics.hubness_permutation_summary, H.summary):
        s = summary(stats, _row(anti=1), _row(anti=0), 3)
        assert (s["n_perm"], s["n_empty"], s["kept"]) == (4, 0, 4)
        assert s["anti_hub_pct"]["diff"] == pytest.approx(100 / 3, rel=1e-15)
        assert s["anti_hub_pct"]["p_two"] == (1 + 3) / 5 and s["anti_hub_pct"]["p_ge"] == (1 + 2) / 5 and s["anti_hub_pct"]["p_le"] == 1.0
        only = summary(stats[:1], _row(anti=1), _row(anti=0), 3)["anti_hub_pct"]
        assert (only["p_two"], only["p_ge"], only["p_le"]) == (1.0, 1.0, 1.0)


def test_summary_by_hand():
    G = 4
    a = _row(S1=8, S2=30, S3=134, anti=1, hubs=1, hub_occ=5, bad=1, good=2, mx=5)       # N = 5 2 1 0
    b = _row(S1=8, S2=16, S3=32, anti=0, hubs=0, hub_occ=0, bad=0, good=6, mx=2)       # N = 2 2 2 2
    x1 = _row(S1=8, S2=18, S3=44, anti=0, hubs=0, hub_occ=0, bad=0, good=4, mx=3)      # N = 3 2 2 1
    y1 = _row(S1=8, S2=22, S3=74, anti=0, hubs=0, hub_occ=0, bad=0, good=4, mx=4)      # N = 4 2 1 1 (hubs need 4 N > 16)
    stats = np.asarray([[a, b],                                                  # the observed labelling itself
                        [b, a],                                                  # its mirror image
                        [x1, y1],
                        [_row(S1=0, S2=0, S3=0, anti=4, mx=0), _row(S1=16)]])    # X is empty: dropped
    # skewness: a = G S2 - S1^2, c = G^2 S3 - 3 G S1 S2 + 2 S1^3
    def skew(m):
        a_, c_ = float(4 * m[1] - m[0] ** 2), float(16 * m[2] - 12 * m[0] * m[1] + 2 * m[0] ** 3)
        return c_ / (a_ * np.sqrt(a_)) if a_ else 0.0
    assert skew(b) == 0.0 and skew(a) == pytest.approx(288 / 56 ** 1.5) and skew(x1) == 0.0 and H.skewness(a, G) == skew(a)
    for summary in (RetrievalMetrics.hubness_permutation_summary, H.summary):
        s = summary(stats, a, b, G, seed=9)
        assert {k: s[k] for k in ("n_perm", "n_empty", "kept", "seed")} == dict(n_perm=4, n_empty=1, kept=3, seed=9)
        assert set(s) == {"n_perm", "n_empty", "kept", "seed"} | set(FIGURES)
        # d_p of skewness: +d0, -d0 exactly (the mirror image), and 0 - skew(y1) = -96 / 24^1.5 = -0.816 beyond -d0 = -0.687
        assert skew(x1) - skew(y1) < -skew(a) < 0
        assert s["skewness"] == dict(diff=skew(a), p_two=1.0, p_ge=(1 + 1) / 4, p_le=1.0)
        assert s["anti_hub_pct"] == dict(diff=25.0, p_two=3 / 4, p_ge=2 / 4, p_le=1.0)           # d_p: 25, -25, 0
        assert s["hub_pct"] == dict(diff=25.0, p_two=3 / 4, p_ge=2 / 4, p_le=1.0)                # d_p: 25, -25, 0
        assert s["bad_hub_pct"] == s["hub_pct"]
        assert s["hub_occurrence_pct"] == dict(diff=62.5, p_two=3 / 4, p_ge=2 / 4, p_le=1.0)     # d_p: 62.5, -62.5, 0
        assert s["good_occurrence_pct"] == dict(diff=-50.0, p_two=3 / 4, p_ge=1.0, p_le=2 / 4)   # d_p: -50, 50, 0
        assert s["max_occurrence"] == dict(diff=3.0, p_two=3 / 4, p_ge=2 / 4, p_le=1.0)          # d_p: 3, -3, -1
    none = RetrievalMetrics.hubness_permutation_summary(stats[3:], a, b, G)
    assert (none["n_empty"], none["kept"]) == (1, 0) and none["skewness"]["p_two"] == 1.0 == none["hub_pct"]["p_two"]
    empty = RetrievalMetrics.hubness_permutation_summary(stats, a, _row(S1=0, S2=0, S3=0, anti=4, mx=0), G)
    assert all(np.isnan(empty[name]["p_two"]) and np.isnan(empty[name]["diff"]) for name in FIGURES)
    for bad in (stats[:, 0], stats[:, :, :8]):
        with pytest.raises(ValueError, match="stats"):
            RetrievalMetrics.hubness_permutation_summary(bad, a, b, G)
    with pytest.raises(ValueError, match="n_gallery"):
        RetrievalMetrics.hubness_permutation_summary(stats, a, b, 0)


def test_summary_equals_the_restatement_and_its_symmetries():
    rng = np.random.default_rng(2)
    G, k, U = 40, 5, 40
    a, b = _lists(rng, U, k, G, 3.0), _lists(rng, U, k, G, 0.5)
    gt = np.arange(U)
    args = (np.arange(U), G, gt, gt + 1)
    ma, mb = (H.moments(*H.counts(x.tolist(), G, gt, gt + 1)) for x in (a, b))
    stats = H.hubness_stats(a, b, *args, seed=3, n_perm=200)
    ab = RetrievalMetrics.hubness_permutation_summary(torch.from_numpy(stats), ma, mb, G, seed=3)
    assert ab == H.summary(stats, ma, mb, G, seed=3)
    assert ab["skewness"]["diff"] > 0 and ab["skewness"]["p_two"] < 0.05
    # swapping A and B swaps the sides: diff negated exactly (skewness too), p_ge and p_le exchanged, p_two kept
    ba = RetrievalMetrics.hubness_permutation_summary(H.hubness_stats(b, a, *args, seed=3, n_perm=200), mb, ma, G, seed=3)
    for name in FIGURES:
        assert ba[name] == dict(diff=-ab[name]["diff"], p_two=ab[name]["p_two"], p_ge=ab[name]["p_le"], p_le=ab[name]["p_ge"]), name


def test_format_hubness_permutation():
    s = {"n_perm": 200, "n_empty": 0, "kept": 200, "seed": 1}
    s.update({name: dict(diff=-0.5 * i, p_two=0.01 * (i + 1), p_ge=1.0, p_le=0.1) for i, name in enumerate(FIGURES)})
    line = RetrievalMetrics.format_hubness_permutation(s, 15, prefix="text->video [DSL] - raw: ")
    assert line.startswith("text->video [DSL] - raw: Hubness@15: skew -0.00 p=0.0100 - anti-hubs -0.50 p=0.0200 - hubs -1.00 p=0.0300")
    assert line.endswith("max N_k -3.00 p=0.0700 (paired permutation test vs raw, 200 permutations)")
    line = RetrievalMetrics.format_hubness_permutation(dict(s, n_empty=3), 5, versus="model")
    assert line.startswith("Hubness@5: ") and line.endswith("(paired permutation test vs model, 200 permutations, 3 empty)")
    seen = []
    RetrievalMetrics(logger=NS(info=seen.append)).log_hubness_permutation(s, 15, prefix="x ")
    RetrievalMetrics().log_hubness_permutation(s, 15)                           # silent without a logger
    assert seen == [RetrievalMetrics.format_hubness_permutation(s, 15, prefix="x ")]


# ---- calibration on the restatement ---------------------------------------------------------------------------------------------------
def test_calibration_of_the_randomisation_test():
    """Null: 300 data sets, U = G = 200, k = 5, A and B the top-k of popularity + independent noise (weight 1.0 both), 200 permutations
    each: skewness's p_two <= 0.05 in at most 27 of them, 0.05 x 300 + 3 binomial standard deviations (3 sqrt(300 x .05 x .95) = 11.3);
    the restatement with these seeds gives 17.  Power: popularity weight 1.0 against 0.5, 50 data sets: p_two <= 0.05 for skewness and
    for anti_hub_pct in at least 45 each; it gives 50 and 50.  hub_pct has little power at this size and gets no bar."""
    U = G = 200
    k, n_perm = 5, 200
    gt = np.arange(U)

    def top_k(rng, pop, weight):
        return np.argsort(-(weight * pop[None, :] + rng.standard_normal((U, G))), axis=1, kind="stable")[:, :k]

    def rejections(trials, wa, wb, data_seed, perm_seed, names):
        count = dict.fromkeys(names, 0)
        for t in range(trials):
            rng = np.random.default_rng(data_seed + t)
            pop = rng.standard_normal(G)
            a, b = top_k(rng, pop, wa), top_k(rng, pop, wb)
            stats = H.single_list_stats(a, b, G, seed=perm_seed + t, n_perm=n_perm)
            ma, mb = (H.moments(*H.counts(x.tolist(), G, gt, gt + 1)) for x in (a, b))
            s = H.summary(stats, ma, mb, G, perm_seed + t, only=names)
            for name in names:
                count[name] += s[name]["p_two"] <= 0.05
        return count
    null = rejections(300, 1.0, 1.0, 0, 1000, ("skewness",))
    power = rejections(50, 1.0, 0.5, 5000, 7000, ("skewness", "anti_hub_pct"))
    print(f"null: {null} of 300 rejected at 0.05; power: {power} of 50")
    assert null["skewness"] <= 27
    assert power["skewness"] >= 45 and power["anti_hub_pct"] >= 45


# ---- the entry point ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    at = header.index("int nr_permtest_hubness(")
    comment, decl = header[header.rindex("/*", 0, at):at], header[at:header.index(");", at)]
    for word in ("s(p, u)", "nr_permtest_rank_stats", "unit_end", "gt_begin", "occ_ab", "[n_perm, 2 (X, Y), 9]", "N G > 2 S1", "N - GN > GN",
                 "LDS", "65 536", "32 768", "NR_EINVAL", "NR_EUNSUPPORTED", "2^24", "2^31 - 1", "NR_OK", "in bounds"):
        assert word in comment, word
    args, res = hip._SIGNATURES["nr_permtest_hubness"]
    assert len(args) == decl.count(",") + 1 == 16 and args[11] is ctypes.c_uint64 and res is ctypes.c_int
    assert [a is ctypes.c_void_p for a in args] == [bool(re.search(r"\*", part)) for part in decl.split(",")]
    assert "nr_permtest_hubness" in hip.exported_symbols() and hasattr(hip.lib(), "nr_permtest_hubness")
    assert (hip.HUBPERM_MAX_GALLERY, hip.HUBPERM_MAX_LISTS) == (32768, 65535) and hip.ABI_VERSION == 5
    # the swap rule lives in the engine's header now, once, and both files take it from there
    csrc = os.path.join(ROOT, "neighborretr_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("nr_resample.h", "nr_permtest.hip", "nr_hubperm.hip")}
    assert "#define NR_PERM_SALT 0x7065726D74657374ull" in text["nr_resample.h"] and "int nr_perm_swap(" in text["nr_resample.h"]
    for f in ("nr_permtest.hip", "nr_hubperm.hip"):
        assert "define NR_PERM_SALT" not in text[f] and "int nr_perm_swap(" not in text[f] and "nr_perm_swap(base, u)" in text[f]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    EINVAL, EUNSUPPORTED = hip.NR_EINVAL, hip.NR_EUNSUPPORTED
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    names = ("idx_a", "idx_b", "n_lists", "k", "unit_end", "U", "G", "gt_begin", "gt_end", "occ_ab", "good_ab", "seed", "p0", "n_perm",
             "out", "stream")
    good = [p, p, 4, 3, p, 3, 10, p, p, p, p, 42, 0, 5, p, None]                 # no device needed: every call returns before a launch

    def call(**over):
        a = list(good)
        for key, v in over.items():
            a[names.index(key)] = v
        return hip.lib().nr_permtest_hubness(*a)
    for name in ("idx_a", "idx_b", "unit_end", "gt_begin", "gt_end", "occ_ab", "good_ab", "out"):
        assert call(**{name: None}) == EINVAL, name
    for U in (0, -1, (1 << 24) + 1):
        assert call(U=U) == EINVAL, U
    for k in (0, -1, 129):
        assert call(k=k) == EINVAL, k
    assert call(n_lists=-1) == EINVAL and call(G=0) == EINVAL and call(G=-5) == EINVAL
    assert call(p0=-1) == EINVAL and call(n_perm=-1) == EINVAL
    assert call(p0=(1 << 31) - 5, n_perm=5) == EINVAL and call(p0=(1 << 31) - 1, n_perm=1) == EINVAL
    # beyond the limits: unsupported, not invalid, and before any launch too
    assert call(G=32769) == EUNSUPPORTED and call(n_lists=65536) == EUNSUPPORTED
    assert call(G=32769, n_perm=0) == EUNSUPPORTED and call(G=32769, k=0) == EINVAL
    # nothing to do: NR_OK without a launch, and the arguments are checked even then
    assert call(n_perm=0) == 0 and call(n_perm=0, p0=(1 << 31) - 1, U=1 << 24, k=128, G=32768, n_lists=65535) == 0
    assert call(n_perm=0, n_lists=0, U=1, k=1, G=1) == 0
    assert call(n_perm=0, k=129) == EINVAL and call(n_perm=0, idx_b=None) == EINVAL


# ---- the evaluator's checks and the command line -----------------------------------------------------------------------------------------
def test_evaluator_checks_hubness_test_before_any_scoring():
    z = torch.zeros((4, 2, 8))
    head = (None, z, z, z[..., 0], z[..., 0], None)                             # no model: nothing may be touched
    with pytest.raises(ValueError, match="hubness_test needs hubness_k > 0 .* and permutation > 0"):
        evaluator.sharded_evaluation(*head, hubness_test=True, permutation=10)
    with pytest.raises(ValueError, match="hubness_test needs hubness_k > 0 .* and permutation > 0"):
        evaluator.sharded_evaluation(*head, hubness_test=1, hubness_k=5)
    for bad in (2, -1, "yes", 0.5, None):
        with pytest.raises(ValueError, match="hubness_test must be 0 or 1"):
            evaluator.sharded_evaluation(*head, hubness_test=bad, hubness_k=5, permutation=10)
    big = torch.zeros((32769, 1, 1))
    with pytest.raises(ValueError, match="32769 items is above the limit of 32768"):
        evaluator.sharded_evaluation(None, big, big, big[..., 0], big[..., 0], None, hubness_test=True, hubness_k=5, permutation=10)


def test_flag_reaches_the_driver_only_when_asked_for():
    from neighborretr_amd import training
    c, kw = evaluator.correction_from_args(NS(test_norm="dsl", permutation=200, hubness_k=5, hubness_test=1), None)
    assert c.key == "test_norm" and kw["hubness_test"] is True and kw["hubness_k"] == 5
    for args in (NS(test_norm="dsl", permutation=200, hubness_k=5), NS(test_norm="dsl", permutation=200, hubness_k=5, hubness_test=0),
                 NS(test_norm="dsl", hubness_test=None)):
        assert "hubness_test" not in evaluator.correction_from_args(args, None)[1]       # off: the driver's arguments are today's
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import main_retrieval
    for eval_epoch in (lambda a: training.eval_epoch(a, None, None, "cpu"), lambda a: main_retrieval.eval_epoch(a, None, None)):
        with pytest.raises(ValueError, match="hubness_test needs hubness_k > 0"):
            eval_epoch(NS(test_norm="dsl", permutation=100, hubness_test=1))
        with pytest.raises(ValueError, match="hubness_test needs hubness_k > 0"):
            eval_epoch(NS(test_norm="dsl", hubness_k=5, hubness_test=1))
        with pytest.raises(ValueError, match="hubness_test must be 0 or 1"):
            eval_epoch(NS(test_norm="dsl", hubness_k=5, permutation=100, hubness_test=3))


def _hub(k=5, G=6, n_lists=4, **over):
    lists = dict(idx=np.zeros((n_lists, k), dtype=np.int32), unit_end=np.arange(n_lists), gt_begin=np.arange(n_lists, dtype=np.int32),
                 gt_end=np.arange(n_lists, dtype=np.int32) + 1)
    lists.update(over)
    return {"k": k, "n_gallery": G, "lists": lists}


def test_compare_evaluations_refuses_lists_that_do_not_pair_up():
    units = dict(entries=np.arange(4), unit_end=np.arange(4), median="mid")
    a = ({"units": units, "hubness": _hub()},) * 2
    for other, word in ((_hub(k=3), r"\(4, 5\) \(k = 5\) and \(4, 3\) \(k = 3\)"), (_hub(G=7), "galleries hold 6 and 7 items"),
                        (_hub(unit_end=np.asarray([0, 0, 2, 3])), "different units or ground-truth ranges"),
                        (_hub(gt_end=np.arange(4, dtype=np.int32) + 2), "different units or ground-truth ranges")):
        with pytest.raises(ValueError, match=word):
            evaluator.compare_evaluations(a, ({"units": units, "hubness": other},) * 2, 10)
    nested = ({"units": units, "test_norm": {"units": units, "hubness": _hub()}},) * 2
    with pytest.raises(ValueError, match="galleries hold 6 and 7 items"):
        evaluator.compare_evaluations(nested, ({"units": units, "test_norm": {"units": units, "hubness": _hub(G=7)}},) * 2, 10)


def test_main_retrieval_accepts_the_flag(monkeypatch, capsys):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main_retrieval

    def parse(argv):
        monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
        return main_retrieval.get_args()
    assert parse([]).hubness_test == 0
    a = parse(["--hubness_test", "1", "--hubness_k", "5", "--permutation", "64", "--test_norm", "dsl"])
    assert (a.hubness_test, a.hubness_k, a.permutation) == (1, 5, 64)
    for argv, word in ((["--hubness_test", "1", "--permutation", "64", "--test_norm", "dsl"], "--hubness_test needs"),
                       (["--hubness_test", "1", "--hubness_k", "5"], "--hubness_test needs"),
                       (["--hubness_test", "2", "--hubness_k", "5", "--permutation", "64", "--test_norm", "dsl"], "--hubness_test")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(argv)
        assert word in capsys.readouterr().err
