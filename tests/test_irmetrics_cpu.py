"""CPU: the restatement of the rank-aware IR metrics (irmetrics_ref) on the worked example, RetrievalMetrics.ir_from_ranks against a
brute-force evaluation that sorts whole lines, the fixed-point bootstrap columns and summaries, the host-side refusals of
nr_pair_ranks / nr_bootstrap_unit_sums and of their wrappers, the evaluator's flag check and the command line."""
import ctypes
import logging
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irmetrics_ref as R
from neighborretr_amd import evaluator, hip, ops, training
from neighborretr_amd.metrics import RetrievalMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ir_from_ranks sums a query's terms with NumPy, the restatement one by one: at most 10 + m terms of size <= 1 per query, each sum
# within a few ulp of the other; 1e-12 on values of size <= 100 is far above that and far below any real difference (>= 1 / m^2 n)
TOL = 1e-12


# ---- the worked example of the definition ------------------------------------------------------------------------------------------
def test_worked_example():
    rr, ap, ndcg, rprec = R.query([0, 2, 5])
    assert abs(ap - 0.7222222222222222) <= 1e-15
    assert abs(rr - 1.0) <= 1e-15
    assert abs(rprec - 2.0 / 3.0) <= 1e-15
    assert abs(R.dcg10([0, 2, 5]) - 1.8562071871080221) <= 1e-15
    assert abs(R.idcg10(3) - 2.1309297535714578) <= 1e-15
    assert abs(ndcg - 0.8710785440003369) <= 1e-15
    # the order of the sentences does not matter, and the product's function gives the same query
    assert R.query([5, 0, 2]) == (rr, ap, ndcg, rprec)
    got = RetrievalMetrics.ir_from_ranks([5, 0, 2], group_end=[3])
    for name, want in zip(R.METRICS, (rr, ap, ndcg, rprec)):
        assert abs(got[name] - 100 * want) <= TOL, name
    assert got["n_queries"] == 1 and got["n_unranked"] == 0 and got["ranks"].tolist() == [5, 0, 2]


def test_more_than_ten_relevant_items_cap_the_ideal_dcg():
    r = list(range(0, 24, 2))                                 # 12 relevant items, five of them below rank 10
    _, _, ndcg, rprec = R.query(r)
    want = sum(1 / np.log2(x + 2) for x in (0, 2, 4, 6, 8)) / sum(1 / np.log2(k + 1) for k in range(1, 11))
    assert abs(ndcg - want) <= 1e-15 and rprec == 6 / 12
    assert abs(RetrievalMetrics.ir_from_ranks(r, [12])["nDCG10"] - 100 * want) <= TOL


# ---- ir_from_ranks against a brute force that sorts whole lines ----------------------------------------------------------------------
def _planted(n_total, V, seed):
    """A matrix with ties along rows and columns, a whole column of one value, both zeros, NaN and +-inf entries and own scores."""
    rng = np.random.default_rng(seed)
    M = rng.integers(-4, 5, size=(n_total, V)).astype(np.float32) / 4            # few distinct values: many ties
    M[rng.random(M.shape) < 0.05] = -0.0
    M[rng.random(M.shape) < 0.05] = 0.0
    M[rng.random(M.shape) < 0.03] = np.nan
    M[rng.random(M.shape) < 0.02] = np.inf
    M[rng.random(M.shape) < 0.02] = -np.inf
    if V > 2:
        M[:, V // 2] = 0.25                                                      # a whole column of one value
    return M


def _sorted_line_query(line, relevant):
    """(RR, AP, nDCG10, RPrec) of one query by sorting its whole line: stable descending order, precision at every hit.  relevant:
    the indices of the ranked relevant entries."""
    order = np.argsort(-np.asarray(line, dtype=np.float32), kind="stable")       # NaN keys sort last: a NaN entry is never ahead
    hit = np.isin(order, relevant)
    where = np.flatnonzero(hit)
    m = len(relevant)
    precision = np.cumsum(hit)[where] / (where + 1.0)
    dcg = np.sum(1.0 / np.log2(where[where < 10] + 2.0))
    idcg = np.sum(1.0 / np.log2(np.arange(1, min(m, 10) + 1) + 1.0))
    return 1.0 / (where[0] + 1.0), precision.mean(), dcg / idcg, hit[:m].sum() / m


def _brute_force(M, ends):
    g = R.groups_of(ends)
    own = M[np.arange(len(g)), g]
    ranked = np.isfinite(own)
    t2v = [_sorted_line_query(M[s], [g[s]]) for s in range(len(g)) if ranked[s]]
    v2t = []
    for v in range(len(ends)):
        rel = np.flatnonzero((g == v) & ranked)
        if len(rel):
            v2t.append(_sorted_line_query(M[:, v], rel))
    return [100 * np.mean(np.asarray(q), axis=0) for q in (t2v, v2t)], int(np.sum(~ranked))


@pytest.mark.parametrize("sizes,seed", [([1] * 23, 1), ([1, 30, 2, 7, 1, 12, 5], 2), ([40], 3), ([3, 1, 1, 4, 1, 2], 4)])
def test_ir_from_ranks_equals_a_brute_force_over_sorted_lines(sizes, seed):
    ends = np.cumsum(sizes)
    M = _planted(int(ends[-1]), len(sizes), seed)
    g = R.groups_of(ends)
    M[0, g[0]], M[-1, g[-1]] = np.nan, np.inf                                    # own scores that leave their pairs unranked
    rt, rv = R.pair_ranks(M, ends)
    (want_t, want_v), n_unranked = _brute_force(M, ends)
    assert 0 < n_unranked < len(rt)                                              # the planted own scores took effect
    for got, want, n_q in ((RetrievalMetrics.ir_from_ranks(rt), want_t, int(np.sum(rt >= 0))),
                           (RetrievalMetrics.ir_from_ranks(rv, ends), want_v, None)):
        for i, name in enumerate(R.METRICS):
            assert abs(got[name] - want[i]) <= 1e-9, name                        # the brute force divides in another order
        assert got["n_unranked"] == n_unranked
        if n_q is not None:
            assert got["n_queries"] == n_q
    # and the product's function equals the restatement's loops
    for ranks, groups in ((rt, None), (rv, ends)):
        got, want = RetrievalMetrics.ir_from_ranks(ranks, groups), R.ir(ranks, groups)
        assert set(got) == set(want) == set(R.METRICS) | {"n_queries", "n_unranked", "ranks"}
        for name in R.METRICS:
            assert abs(got[name] - want[name]) <= TOL, name
        assert got["n_queries"] == want["n_queries"] and got["n_unranked"] == want["n_unranked"]
        assert np.array_equal(got["ranks"], want["ranks"]) and got["ranks"].dtype == np.int64


def test_the_restatement_gives_the_ranked_pairs_of_one_line_distinct_ranks():
    """A check of the yardstick itself, not of product code: the GPU test asks the same of the kernel's ranks."""
    ends = np.cumsum([6, 9, 1, 14])
    rt, rv = R.pair_ranks(_planted(30, 4, 9), ends)
    begin = 0
    for end in ends:
        kept = rv[begin:end][rv[begin:end] >= 0]
        assert len(set(kept.tolist())) == len(kept)
        begin = end


def test_one_relevant_item_gives_map_equal_to_mrr():
    rng = np.random.default_rng(11)
    ranks = rng.integers(-1, 40, 200)
    for groups in (None, np.arange(1, 201)):                                     # m = 1 on both sides of a single-sentence set
        got = RetrievalMetrics.ir_from_ranks(ranks, groups)
        assert got["mAP"] == got["MRR"] and got["n_queries"] == int(np.sum(ranks >= 0))
    a, b = RetrievalMetrics.ir_from_ranks(ranks), RetrievalMetrics.ir_from_ranks(ranks, np.arange(1, 201))
    for name in R.METRICS:
        assert abs(a[name] - b[name]) <= TOL, name


def test_rprec_is_recall_at_one_on_a_tie_free_single_sentence_set():
    rng = np.random.default_rng(12)
    M = rng.permutation(31 * 31).reshape(31, 31).astype(np.float32)              # distinct values: no ties
    assert len(np.unique(M)) == M.size
    ends = np.arange(1, 32)
    rt, rv = R.pair_ranks(M, ends)
    greater_t = (M > np.diag(M)[:, None]).sum(1)
    greater_v = (M > np.diag(M)[None, :]).sum(0)
    for ranks, greater in ((rt, greater_t), (rv, greater_v)):
        assert np.array_equal(ranks, greater)
        r1 = RetrievalMetrics.metrics_from_ranks(greater)["R1"]
        assert abs(RetrievalMetrics.ir_from_ranks(ranks, ends)["RPrec"] - r1) <= TOL
        assert abs(RetrievalMetrics.ir_from_ranks(ranks)["RPrec"] - r1) <= TOL


def test_a_video_whose_sentences_are_all_unranked_is_dropped_and_counted():
    ranks = np.asarray([0, 3, -1, -1, -1, 2, -7])                                # videos of 2, 2, 3 sentences; the second is unranked
    got = RetrievalMetrics.ir_from_ranks(ranks, [2, 4, 7])
    assert got["n_queries"] == 2 and got["n_unranked"] == 4 and got["ranks"].tolist() == [0, 3, -1, -1, -1, 2, -1]
    want = [np.mean([a, b]) * 100 for a, b in zip(R.query([0, 3]), R.query([2]))]
    for name, w in zip(R.METRICS, want):
        assert abs(got[name] - w) <= TOL, name
    # text->video: the unranked sentences are dropped one by one
    assert RetrievalMetrics.ir_from_ranks(ranks)["n_queries"] == 3
    # nothing ranked at all: no query, NaN means
    none = RetrievalMetrics.ir_from_ranks([-1, -1], [1, 2])
    assert none["n_queries"] == 0 and none["n_unranked"] == 2 and all(np.isnan(none[name]) for name in R.METRICS)
    for bad in ([2, 1, 7], [2, 4, 6], [-1, 4, 7], [], [2, 2, 7], [0, 4, 7]):       # the last two: a video without a sentence
        with pytest.raises(ValueError, match="group_end"):
            RetrievalMetrics.ir_from_ranks(ranks, bad)


# ---- the bootstrap's fixed-point columns and summaries --------------------------------------------------------------------------------
def _case(seed=21, sizes=(3, 1, 6, 2, 2, 9, 1)):
    ends = np.cumsum(sizes)
    rt, rv = R.pair_ranks(_planted(int(ends[-1]), len(sizes), seed), ends)
    return rt, rv, ends


def test_unit_columns_equal_the_restatement_and_a_direct_mean():
    rt, rv, ends = _case()
    for ranks, groups, units in ((rt, None, None), (rt, None, ends), (rv, ends, None)):
        cols = RetrievalMetrics.ir_unit_columns(ranks, groups, units)
        assert cols.dtype == np.int64 and np.array_equal(cols, R.unit_columns(ranks, groups, units))
        direct = RetrievalMetrics.ir_from_ranks(ranks, groups)
        tot = cols.sum(axis=0)
        assert tot[0] == direct["n_queries"]
        for i, name in enumerate(R.METRICS):                                     # every query rounds by at most 2^-33
            assert abs(tot[1 + i] / (R.ONE * tot[0]) - direct[name] / 100) <= 2.0 ** -32, name
    units = RetrievalMetrics.ir_unit_columns(rt, None, ends)
    assert units.shape == (len(ends), 5) and units[:, 0].sum() == int(np.sum(rt >= 0))
    with pytest.raises(ValueError, match="unit_end"):
        RetrievalMetrics.ir_unit_columns(rv, ends, ends)


def test_bootstrap_summary_agrees_with_direct_means_of_the_resamples():
    rt, rv, ends = _case(22)
    import bootstrap_ref as B
    for ranks, groups, units, seed in ((rt, None, ends, 5), (rv, ends, None, 6)):
        cols = RetrievalMetrics.ir_unit_columns(ranks, groups, units)
        n_boot = 40
        sums = R.unit_sums(cols, seed=seed, n_boot=n_boot)
        got = RetrievalMetrics.ir_bootstrap_summary(sums, cols, level=0.9)
        assert got["n_boot"] == n_boot and got["level"] == 0.9 and got["n_empty"] == int(np.sum(sums[:, 0] == 0))
        # a direct fp64 evaluation of every resample: the drawn units' queries, one mean
        per_query = {slot: v for slot, v in R.queries(ranks, groups)}
        unit_of = np.searchsorted(units, np.arange(len(ranks)), side="right") if units is not None else np.arange(len(cols))
        direct = {name: [] for name in R.METRICS}
        for b in range(n_boot):
            drawn = B.draws(seed, b, len(cols))
            vals = [per_query[slot] for u in drawn for slot in np.flatnonzero(unit_of == u) if slot in per_query]
            if vals:
                for i, name in enumerate(R.METRICS):
                    direct[name].append(100 * np.mean([v[i] for v in vals]))
        want = R.resampled(sums)
        for name in R.METRICS:
            x = np.asarray(direct[name])
            assert len(x) == n_boot - got["n_empty"] and np.array_equal(want[name], RetrievalMetrics._ir_values(sums)[0][name][sums[:, 0] > 0])
            assert np.abs(want[name] - x).max() <= 100 * 2.0 ** -32
            lo, hi = np.percentile(want[name], [100 * (1 - 0.9) / 2, 100 * (1 + 0.9) / 2])
            assert got[name]["lo"] == lo and got[name]["hi"] == hi and got[name]["se"] == float(np.std(want[name]))
            assert abs(got[name]["point"] - RetrievalMetrics.ir_from_ranks(ranks, groups)[name]) <= 100 * 2.0 ** -32


def test_empty_resamples_are_dropped_and_counted():
    cols = np.asarray([[0, 0, 0, 0, 0], [1, R.ONE, R.ONE // 2, R.ONE, 0]], dtype=np.int64)
    sums = np.asarray([[0, 0, 0, 0, 0], [2, 2 * R.ONE, R.ONE, 2 * R.ONE, 0], [1, R.ONE, R.ONE // 2, R.ONE, 0]], dtype=np.int64)
    got = RetrievalMetrics.ir_bootstrap_summary(sums, cols)
    assert got["n_boot"] == 3 and got["n_empty"] == 1
    assert got["MRR"] == {"point": 100.0, "se": 0.0, "lo": 100.0, "hi": 100.0}
    assert got["mAP"]["point"] == 50.0 and got["RPrec"]["point"] == 0.0
    none = RetrievalMetrics.ir_bootstrap_summary(sums[:1], cols)
    assert none["n_empty"] == 1 and np.isnan(none["MRR"]["lo"]) and none["MRR"]["point"] == 100.0
    with pytest.raises(ValueError, match="sums must be"):
        RetrievalMetrics.ir_bootstrap_summary(sums[:, :4], cols)
    with pytest.raises(ValueError, match="level"):
        RetrievalMetrics.ir_bootstrap_summary(sums, cols, level=1.0)


def test_paired_summary_is_corrected_minus_raw_on_the_same_draws():
    rt, rv, ends = _case(23)
    rt2, rv2, _ = _case(24)
    a, b = RetrievalMetrics.ir_unit_columns(rv2, ends), RetrievalMetrics.ir_unit_columns(rv, ends)
    sums = R.unit_sums(np.concatenate([a, b], axis=1), seed=3, n_boot=25)
    assert np.array_equal(sums[:, :5], R.unit_sums(a, seed=3, n_boot=25)) and np.array_equal(sums[:, 5:], R.unit_sums(b, seed=3, n_boot=25))
    got = RetrievalMetrics.ir_paired_bootstrap_summary(sums, a, b, level=0.8)
    keep = (sums[:, 0] > 0) & (sums[:, 5] > 0)
    assert got["n_boot"] == 25 and got["n_empty"] == int(np.sum(~keep)) and got["level"] == 0.8
    one, raw = RetrievalMetrics.ir_bootstrap_summary(sums[:, :5], a), RetrievalMetrics.ir_bootstrap_summary(sums[:, 5:], b)
    for i, name in enumerate(R.METRICS):
        d = 100.0 * sums[keep, 1 + i] / (float(R.ONE) * sums[keep, 0]) - 100.0 * sums[keep, 6 + i] / (float(R.ONE) * sums[keep, 5])
        assert got[name]["point"] == one[name]["point"] - raw[name]["point"]
        lo, hi = np.percentile(d, [100 * (1 - 0.8) / 2, 100 * (1 + 0.8) / 2])
        assert got[name]["se"] == float(np.std(d)) and got[name]["lo"] == lo and got[name]["hi"] == hi
        assert got[name]["frac_le0"] == float(np.mean(d <= 0)) and got[name]["frac_ge0"] == float(np.mean(d >= 0))
    with pytest.raises(ValueError, match="paired sums"):
        RetrievalMetrics.ir_paired_bootstrap_summary(sums[:, :5], a, b)


def test_format_and_log_ir(caplog):
    ir = {"MRR": 45.12, "mAP": 45.1, "nDCG10": 50.24, "RPrec": 33.04, "n_queries": 9, "n_unranked": 0}
    assert RetrievalMetrics.format_ir(ir, prefix="Text-to-Video: ") == "Text-to-Video: MRR 45.1 - mAP 45.1 - nDCG@10 50.2 - R-Prec 33.0"
    iv = {"point": 45.1, "se": 1.0, "lo": 43.0, "hi": 47.25}
    summary = dict({name: dict(iv) for name in R.METRICS}, n_boot=200, n_empty=0, level=0.95)
    line = RetrievalMetrics.format_ir_bootstrap(summary, prefix="x: ")
    assert line.startswith("x: MRR 45.1 [43.0, 47.2] - mAP 45.1 [43.0, 47.2] - nDCG@10") and line.endswith("(95% bootstrap, 200 resamples)")
    paired = dict({name: dict(iv, point=-0.5, lo=-1.0, hi=0.25, frac_le0=0.9, frac_ge0=0.1) for name in R.METRICS}, n_boot=200, n_empty=3,
                  level=0.9)
    line = RetrievalMetrics.format_ir_bootstrap(paired)
    assert line.startswith("MRR -0.5 [-1.0, +0.2] frac<=0 0.900 - mAP") and line.endswith("(90% paired bootstrap vs raw, 200 resamples, 3 empty)")
    logger = logging.getLogger("ir_test")
    with caplog.at_level(logging.INFO, logger="ir_test"):
        RetrievalMetrics(logger=logger).log_ir(dict(ir, bootstrap=summary, bootstrap_vs_raw=paired), prefix="Video-to-Text [DSL b=20]: ")
    lines = [r.getMessage() for r in caplog.records]
    assert len(lines) == 3 and all(l.startswith("Video-to-Text [DSL b=20]: MRR ") for l in lines)
    RetrievalMetrics().log_ir(ir)                                                # silent without a logger


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    for name in ("nr_pair_ranks", "nr_bootstrap_unit_sums"):
        assert f"int {name}(" in header and name in hip.exported_symbols() and hasattr(hip.lib(), name), name
    comment = header[header.index("/* Ranks of every relevant"):header.index("int nr_pair_ranks(")]
    for word in ("group_end", "own", "AHEAD", "NaN", "unranked", "row_rank", "col_ahead", "Overwritten", "NULL", "NR_EINVAL", "NR_OK"):
        assert word in comment, word
    comment = header[header.index("/* Bootstrap of per-unit sums"):header.index("int nr_bootstrap_unit_sums(")]
    for word in ("[U, Q]", "2^24", "16", "nr_bootstrap_rank_stats", "2^62", "NR_EINVAL", "NR_OK"):
        assert word in comment, word
    assert hip.ABI_VERSION == 5 and hip.version() == 5
    assert (hip.BOOT_MAX_COLS, hip.BOOT_SUM_LIMIT) == (16, 1 << 62)
    args, res = hip._SIGNATURES["nr_pair_ranks"]
    assert len(args) == 10 and res is ctypes.c_int
    args, res = hip._SIGNATURES["nr_bootstrap_unit_sums"]
    assert len(args) == 8 and args[3] is ctypes.c_uint64 and res is ctypes.c_int


def test_pair_ranks_refuses_bad_arguments_before_any_launch():
    fn = hip.lib().nr_pair_ranks                              # host-side checks: no device needed
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    names = ("M", "n_rows", "V", "row0", "n_total", "group_end", "own", "row_rank", "col_ahead", "stream")
    good = [p, 4, 3, 2, 8, p, p, p, p, None]

    def call(**over):
        a = list(good)
        for k, v in over.items():
            a[names.index(k)] = v
        return fn(*a)
    for name in ("M", "group_end", "own"):                                       # a null required pointer
        assert call(**{name: None}) == hip.NR_EINVAL, name
    for over in (dict(n_rows=-1), dict(V=0), dict(V=-2), dict(row0=-1), dict(n_total=-1), dict(row0=5), dict(n_rows=7),
                 dict(row0=(1 << 31) - 1, n_rows=(1 << 31) - 1, n_total=(1 << 31) - 1)):
        assert call(**over) == hip.NR_EINVAL, over
    # an empty slab with nothing to zero: NR_OK without a launch, and M may be NULL then; its arguments are checked even so
    assert call(n_rows=0, col_ahead=None) == 0 and call(n_rows=0, col_ahead=None, M=None, row_rank=None) == 0
    assert call(n_rows=0, row0=8, col_ahead=None) == 0
    assert call(n_rows=0, row0=9, col_ahead=None) == hip.NR_EINVAL and call(n_rows=0, col_ahead=None, own=None) == hip.NR_EINVAL


def test_bootstrap_unit_sums_refuses_bad_arguments_before_any_launch():
    fn = hip.lib().nr_bootstrap_unit_sums
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    names = ("values", "U", "Q", "seed", "b0", "n_boot", "out", "stream")
    good = [p, 7, 5, 42, 0, 3, p, None]

    def call(**over):
        a = list(good)
        for k, v in over.items():
            a[names.index(k)] = v
        return fn(*a)
    assert call(values=None) == hip.NR_EINVAL and call(out=None) == hip.NR_EINVAL
    for U in (0, -1, (1 << 24) + 1):
        assert call(U=U) == hip.NR_EINVAL, U
    for Q in (0, -1, 17):
        assert call(Q=Q) == hip.NR_EINVAL, Q
    assert call(b0=-1) == hip.NR_EINVAL and call(n_boot=-1) == hip.NR_EINVAL
    assert call(b0=(1 << 31) - 5, n_boot=5) == hip.NR_EINVAL
    assert call(n_boot=0) == 0 and call(n_boot=0, U=1 << 24, Q=16) == 0 and call(n_boot=0, b0=(1 << 31) - 1) == 0
    assert call(n_boot=0, Q=17) == hip.NR_EINVAL                                 # arguments are checked even then


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    M, ge, own = torch.zeros((2, 3)), torch.tensor([1, 2, 4], dtype=torch.int32), torch.zeros((4,))
    with pytest.raises(ValueError, match="on the GPU"):
        ops.pair_ranks(M, 0, ge, own)
    with pytest.raises(ValueError, match="on the GPU"):
        ops.bootstrap_unit_sums(torch.zeros((3, 5), dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        ops.bootstrap_unit_sums(torch.zeros((3, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        ops.bootstrap_unit_sums(torch.zeros((15,), dtype=torch.int64))


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_evaluator_checks_the_flag_before_any_work():
    assert evaluator._check_ir(False) is False and evaluator._check_ir(0) is False
    assert evaluator._check_ir(True) is True and evaluator._check_ir(1) is True and evaluator._check_ir(np.int64(1)) is True
    for bad in (2, -1, 0.5, 1.0, "1", "yes", None, [1]):
        with pytest.raises(ValueError, match="ir_metrics must be 0 or 1"):
            evaluator._check_ir(bad)
    z = torch.zeros((4, 2, 8))
    for fn, extra in ((evaluator.sharded_metrics, ()), (evaluator.sharded_multi_sentence_metrics, ([0, 1, 2, 3],)),
                      (evaluator.sharded_metrics_with_hubness, (5,)), (evaluator.sharded_metrics_with_test_norm, ("is",)),
                      (evaluator.sharded_metrics_with_local_scaling, ("csls",)),
                      (evaluator.sharded_metrics_with_mutual_proximity, ("emp",))):
        head = (None, z, z, z[..., 0], z[..., 0])
        pos = head + extra + (None,) if fn is evaluator.sharded_multi_sentence_metrics else head + (None,) + extra
        with pytest.raises(ValueError, match="ir_metrics must be 0 or 1"):       # before any scoring: there is no model
            fn(*pos, ir=2)


def test_both_eval_epochs_refuse_a_bad_flag_before_any_work():
    sys.path.insert(0, ROOT)
    import main_retrieval
    for bad in (2, -1, 0.5, "on"):
        with pytest.raises(ValueError, match="ir_metrics must be 0 or 1"):
            training.eval_epoch(SimpleNamespace(ir_metrics=bad), None, None, "cpu")      # no model, no loader: nothing may be touched
        with pytest.raises(ValueError, match="ir_metrics must be 0 or 1"):
            main_retrieval.eval_epoch(SimpleNamespace(ir_metrics=bad), None, None)


def test_main_retrieval_accepts_the_flag(monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import main_retrieval

    def parse(argv):
        monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
        return main_retrieval.get_args()
    assert parse([]).ir_metrics == 0
    a = parse(["--ir_metrics", "1", "--bootstrap", "50", "--test_norm", "dsl"])
    assert (a.ir_metrics, a.bootstrap, a.test_norm) == (1, 50, "dsl")
    for bad in ("2", "-1", "yes"):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(["--ir_metrics", bad])
        assert "--ir_metrics" in capsys.readouterr().err
