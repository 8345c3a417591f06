"""GPU: nr_permtest_rank_stats and nr_permtest_unit_sums against their restatement (permtest_ref) integer for integer, their
independence of how the permutations are split over calls, the invariants of the two sides, the wrappers' refusals, the
"permutation_vs_raw" entries of the sharded evaluator on one and on three emulated ranks, evaluator.compare_evaluations, and the log
lines of main_retrieval.py with --permutation and --compare_model."""
import copy
import functools
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import permtest_ref as P
from neighborretr_amd import evaluator, ops, training
from neighborretr_amd.metrics import RetrievalMetrics
from test_evaldriver_gpu import _bank, _sets
from test_irmetrics_gpu import DEV, N, _emulated, _model, _same_tree, _testset, _without

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = (1, 5, 10, 50)
CUTS8 = (1, 2, 3, 5, 10, 50, 100, 299)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def _gpu(a, b, **kw):
    out = ops.permtest_rank_stats(_i32(a[0]), _i32(a[1]), _i32(b[0]), _i32(b[1]), **kw)
    assert out.dtype == torch.int64 and out.is_cuda
    return out.cpu().numpy()


def _gpu_sums(va, vb, **kw):
    out = ops.permtest_unit_sums(_i64(va), _i64(vb), **kw)
    assert out.dtype == torch.int64 and out.is_cuda
    return out.cpu().numpy()


def _single(rng, U, high):
    """(ranks, unit_end): U units of one entry each with ranks below `high`."""
    return rng.integers(0, high, U), np.arange(U)


def _multi(rng, U, high, empty=()):
    """(ranks, unit_end): U units of 0 to 5 entries with ranks below `high`; the units listed in `empty` hold none."""
    size = rng.integers(0, 6, U)
    size[list(empty)] = 0
    return rng.integers(0, high, int(size.sum())), np.cumsum(size) - 1


def _nothing(U):
    """A ranking whose units are all empty."""
    return np.zeros((0,), dtype=np.int64), np.full(U, -1)


# ---- the rank kernel against the restatement -----------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(2025)
    c = {}
    c["U1"] = dict(a=([4, 4, 9], [2]), b=([7], [0]))
    c["U1_b_empty"] = dict(a=([3], [0]), b=_nothing(1))
    c["U2"] = dict(a=([6, 1, 2000], [0, 2]), b=([5], [-1, 0]))
    c["worked_example"] = dict(a=([0, 3, 3, 70000, 1, 0, 12], [0, 2, 2, 3, 6]), b=([0, 0, 5, 2, 9], [0, 1, 2, 3, 4]), seed=42)
    c["U63_single_one_pass"] = dict(a=_single(rng, 63, 1024), b=_single(rng, 63, 40), seed=5)
    c["U64_units_of_0_to_5_two_passes"] = dict(a=_multi(rng, 64, 1 << 12, empty=(0, 63)), b=_multi(rng, 64, 1025, empty=(0,)), seed=6)
    c["U257_three_passes_K8"] = dict(a=_multi(rng, 257, 1 << 30, empty=(256,)), b=_multi(rng, 257, 300), cuts=CUTS8, seed=2)
    c["U257_K1"] = dict(a=_single(rng, 257, 20), b=_multi(rng, 257, 20), cuts=(3,))
    c["U1000_single_one_pass"] = dict(a=_single(rng, 1000, 1000), b=_single(rng, 1000, 1000), seed=7)
    c["U1000_units_of_0_to_5_two_passes"] = dict(a=_multi(rng, 1000, 1 << 20, empty=(0, 999)), b=_multi(rng, 1000, 1 << 11), seed=8)
    c["every_unit_of_b_empty"] = dict(a=_multi(rng, 64, 5000), b=_nothing(64))
    c["every_unit_of_a_empty"] = dict(a=_nothing(257), b=_single(rng, 257, 1 << 21), cuts=CUTS8)
    c["both_empty"] = dict(a=_nothing(9), b=_nothing(9))
    c["all_ranks_equal"] = dict(a=(np.full(300, 77), np.arange(300)), b=(np.full(600, 77), 2 * np.arange(300) + 1))
    c["all_ranks_equal_and_large"] = dict(a=(np.full(63, 1 << 29), np.arange(63)), b=(np.full(63, 1 << 29), np.arange(63)))
    c["position_n_half_needs_the_successor"] = dict(a=(np.arange(6) * 1000, np.arange(6)), b=(np.arange(6) * 1000 + 500, np.arange(6)))
    c["largest_ranks"] = dict(a=([(1 << 30) - 1, 0, (1 << 30) - 1, (1 << 30) - 2, 1 << 20, 1023, 1024], [1, 2, 4, 6]),
                              b=([(1 << 20) - 1, 1 << 10, (1 << 30) - 1], [0, 0, 1, 2]))
    c["largest_seed_late_p0"] = dict(a=_multi(rng, 70, 90), b=_multi(rng, 70, 2000), seed=(1 << 64) - 1, p0=(1 << 31) - 1 - 64)
    for case in c.values():
        case.setdefault("n_perm", 64)
    c["U257_three_passes_K8"]["n_perm"] = 256                    # more permutations than one wave of workgroups
    return c


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_rank_kernel_equals_the_restatement_integer_for_integer(name):
    case = dict(CASES[name])
    a, b = case.pop("a"), case.pop("b")
    want = P.rank_stats(a[0], a[1], b[0], b[1], **case)
    got = _gpu(a, b, **case)
    assert got.shape == want.shape == (case["n_perm"], 2, 4 + len(case.get("cuts", CUTS)))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # the two sides hold every entry of both rankings exactly once
    total = np.asarray(P.entry_stats(list(a[0]) + list(b[0]), case.get("cuts", CUTS)))
    keep = [0, 1] + list(range(4, got.shape[2]))
    assert (got[:, 0, keep] + got[:, 1, keep] == total[keep]).all()
    if name == "worked_example":
        assert got[0].tolist() == [[6, 70013, 0, 1, 3, 4, 4, 5], [6, 22, 3, 3, 1, 4, 6, 6]]
    if name == "both_empty":
        assert (got == [0, 0, -1, -1, 0, 0, 0, 0]).all()
    if name in ("U1_b_empty", "every_unit_of_b_empty", "every_unit_of_a_empty"):
        assert (got[:, :, 0] == 0).any() if name == "U1_b_empty" else (got[:, :, 0] > 0).all()
        assert ((got[:, :, 0] == 0) == (got[:, :, 2] == -1)).all() and ((got[:, :, 0] == 0) == (got[:, :, 3] == -1)).all()
    if name == "position_n_half_needs_the_successor":
        assert (got[:, :, 2] < got[:, :, 3]).all()                                    # twelve distinct values, six a side
    if name.startswith("all_ranks_equal"):
        assert (got[:, :, 2] == got[:, :, 3]).all() and len(set(got[:, :, 2].reshape(-1).tolist())) == 1
    if name == "U1000_units_of_0_to_5_two_passes":
        assert (got[:, :, 2] >= 1024).any()                                            # the select went past its first digit


def test_any_split_over_p0_gives_the_same_integers():
    rng = np.random.default_rng(8)
    a, b = _multi(rng, 257, 1 << 12), _multi(rng, 257, 1 << 22)
    whole = _gpu(a, b, seed=77, p0=0, n_perm=70)
    parts = [_gpu(a, b, seed=77, p0=0, n_perm=1), _gpu(a, b, seed=77, p0=1, n_perm=5), _gpu(a, b, seed=77, p0=6, n_perm=0),
             _gpu(a, b, seed=77, p0=6, n_perm=64)]
    assert parts[2].shape == (0, 2, 8) and np.array_equal(whole, np.concatenate(parts))
    assert not np.array_equal(whole, _gpu(a, b, seed=78, n_perm=70))
    assert np.array_equal(_gpu(b, a, seed=77, n_perm=70), whole[:, ::-1])             # the rankings exchanged: the sides exchanged
    assert np.array_equal(_gpu(a, b)[:5], P.rank_stats(*a, *b, n_perm=5))              # the defaults: cuts 1 5 10 50, seed 0, p0 0
    assert _gpu(a, b, cuts=(2,)).shape == (1000, 2, 5)


# ---- the unit sums against the restatement -------------------------------------------------------------------------------------------------
def _values(rng, U, Q):
    return rng.integers(-(1 << 40), 1 << 40, (U, Q))


@pytest.mark.parametrize("Q", [1, 5, 10, 16])
@pytest.mark.parametrize("U", [1, 2, 63, 64, 257, 1000])
def test_unit_sums_equal_the_restatement_integer_for_integer(U, Q):
    rng = np.random.default_rng(100 * U + Q)
    va, vb = _values(rng, U, Q), _values(rng, U, Q)
    assert (va < 0).any() and (vb < 0).any() or U * Q < 4
    seed, p0, n_perm = 31 + Q, U % 7, 64
    want = P.unit_sums(va, vb, seed=seed, p0=p0, n_perm=n_perm)
    got = _gpu_sums(va, vb, seed=seed, p0=p0, n_perm=n_perm)
    assert got.shape == (n_perm, Q) and np.array_equal(got, want), np.argwhere(got != want)[:8]
    # side Y = total_a + total_b - X is the sums with the inputs exchanged
    assert np.array_equal(_gpu_sums(vb, va, seed=seed, p0=p0, n_perm=n_perm), (va.sum(0) + vb.sum(0))[None, :] - got)


def test_unit_sums_with_a_large_seed_a_late_p0_and_a_split_over_calls():
    rng = np.random.default_rng(3)
    va, vb = _values(rng, 257, 10), -_values(rng, 257, 10)
    seed, p0 = (1 << 64) - 2, (1 << 31) - 1 - 70
    want = P.unit_sums(va, vb, seed=seed, p0=p0, n_perm=70)
    assert np.array_equal(_gpu_sums(va, vb, seed=seed, p0=p0, n_perm=70), want)
    pieces = [_gpu_sums(va, vb, seed=seed, p0=p0, n_perm=1), _gpu_sums(va, vb, seed=seed, p0=p0 + 1, n_perm=5),
              _gpu_sums(va, vb, seed=seed, p0=p0 + 6, n_perm=0), _gpu_sums(va, vb, seed=seed, p0=p0 + 6, n_perm=64)]
    assert pieces[2].shape == (0, 10) and np.array_equal(np.concatenate(pieces), want)
    assert np.array_equal(_gpu_sums(va[:, :5], vb[:, :5], seed=seed, p0=p0, n_perm=70), want[:, :5])     # columns are independent
    big = np.zeros((4, 3), dtype=np.int64)
    big[2, 1] = (1 << 60) - 1                                                    # U max|value| just below 2^62: accepted and exact
    assert np.array_equal(_gpu_sums(big, -big, seed=1, n_perm=64), P.unit_sums(big, -big, seed=1, n_perm=64))


@pytest.mark.parametrize("U", [1, 2, 63, 64, 257, 1000])
def test_both_kernels_use_the_same_swap_bits(U):
    """Ranking a: one entry per unit; ranking b: nothing.  n_X counts the units with s = 0, as does side X of a column of ones
    against a column of zeros; with the rankings exchanged both count the units with s = 1."""
    ranks = (np.arange(U) % 5, np.arange(U))
    ones, zeros = np.ones((U, 1), dtype=np.int64), np.zeros((U, 1), dtype=np.int64)
    seed, p0, n_perm = 1234, 3, 128
    stats = _gpu(ranks, _nothing(U), cuts=(1,), seed=seed, p0=p0, n_perm=n_perm)
    sums = _gpu_sums(ones, zeros, seed=seed, p0=p0, n_perm=n_perm)
    assert np.array_equal(sums[:, 0], stats[:, 0, 0]) and np.array_equal(U - sums[:, 0], stats[:, 1, 0])
    assert np.array_equal(sums[:, 0], U - P.swap_matrix(seed, p0, n_perm, U).sum(1))
    back = _gpu(_nothing(U), ranks, cuts=(1,), seed=seed, p0=p0, n_perm=n_perm)
    assert np.array_equal(_gpu_sums(zeros, ones, seed=seed, p0=p0, n_perm=n_perm)[:, 0], back[:, 0, 0])
    if U >= 63:
        assert 0 < sums[:, 0].min() and sums[:, 0].max() < U and len(set(sums[:, 0].tolist())) > 3


# ---- the wrappers' refusals ------------------------------------------------------------------------------------------------------------------
def test_rank_stats_wrapper_refuses_bad_arguments():
    r, e = _i32([0, 3, 2]), _i32([0, 2])
    assert ops.permtest_rank_stats(r, e, r, e, n_perm=2).shape == (2, 2, 8)
    assert ops.permtest_rank_stats(r, e, r, e, n_perm=0).shape == (0, 2, 8)
    bad = [
        dict(ranks_a=r.long()), dict(ranks_a=r.cpu()), dict(unit_end_a=e.cpu()), dict(unit_end_b=e.float()), dict(ranks_b=r.cpu()),
        dict(ranks_a=_i32([0, -1, 2])), dict(ranks_b=_i32([0, 1 << 30, 2])),                                  # ranks outside [0, 2^30)
        dict(unit_end_a=_i32([2, 0])), dict(unit_end_b=_i32([0, 1])), dict(unit_end_a=_i32([0, 3])),            # decreasing / not E - 1
        dict(unit_end_b=_i32([-2, 2])), dict(unit_end_a=_i32([])), dict(unit_end_b=_i32([0, 1, 2])),            # b: the same U units
        dict(ranks_b=None), dict(unit_end_b=None),                                                              # both rankings are required
        dict(cuts=(5, 1)), dict(cuts=(1, 1)), dict(cuts=(0, 5)), dict(cuts=()), dict(cuts=tuple(range(1, 10))), dict(cuts=(1.5,)),
        dict(p0=-1), dict(n_perm=-1), dict(p0=(1 << 31) - 2, n_perm=2), dict(seed=-1), dict(seed=1 << 64), dict(n_perm=2.5),
    ]
    for over in bad:
        kw = dict(ranks_a=r, unit_end_a=e, ranks_b=r, unit_end_b=e, n_perm=2)
        kw.update(over)
        with pytest.raises(ValueError):
            ops.permtest_rank_stats(**kw)


def test_unit_sums_wrapper_refuses_bad_arguments():
    v = _i64(np.arange(12).reshape(4, 3))
    assert ops.permtest_unit_sums(v, v, n_perm=2).shape == (2, 3) and ops.permtest_unit_sums(v, v, n_perm=0).shape == (0, 3)
    big = np.zeros((4, 3), dtype=np.int64)
    big[2, 1] = 1 << 60                                                          # U max|value| = 2^62, in either input, either sign
    for over in (dict(values_a=_i64(big)), dict(values_b=_i64(big)), dict(values_a=_i64(-big)), dict(values_b=_i64(-big))):
        with pytest.raises(ValueError, match="2\\^62"):
            ops.permtest_unit_sums(**dict(dict(values_a=v, values_b=v, n_perm=2), **over))
    bad = [dict(values_a=v.int()), dict(values_b=v.cpu()), dict(values_a=v[0]), dict(values_b=v[:3]), dict(values_b=v[:, :2]),
           dict(values_a=_i64(np.zeros((3, 17))), values_b=_i64(np.zeros((3, 17)))), dict(values_a=None),
           dict(values_a=_i64(np.zeros((0, 3))), values_b=_i64(np.zeros((0, 3)))),
           dict(seed=-1), dict(seed=1 << 64), dict(p0=-1), dict(n_perm=-1), dict(p0=(1 << 31) - 2, n_perm=2), dict(n_perm=2.5)]
    for over in bad:
        with pytest.raises(ValueError):
            ops.permtest_unit_sums(**dict(dict(values_a=v, values_b=v, n_perm=2), **over))


# ---- the sharded evaluator ------------------------------------------------------------------------------------------------------------------
NP, SEED = 64, 11
PERM = dict(permutation=NP, permutation_seed=SEED)
ARGS = SimpleNamespace(world_size=1)
RECORDS = {"dsl": lambda: evaluator.test_norm_correction("dsl", 12.5), "csls": lambda: evaluator.local_scaling_correction("csls", 3),
           "emp": lambda: evaluator.mutual_proximity_correction("emp")}


def _want_rank_summary(units, other, seed):
    stats = P.rank_stats(units["entries"], units["unit_end"], other["entries"], other["unit_end"], CUTS, seed=seed, n_perm=NP)
    return P.permutation_summary(stats, CUTS, units["entries"], other["entries"], units["median"], seed=seed)


def _want_ir_summary(columns, other, seed):
    return P.ir_permutation_summary(P.unit_sums(columns, other, seed=seed, n_perm=NP), columns, other, seed=seed)


@pytest.mark.parametrize("kind", ["single", "multi"])
@pytest.mark.parametrize("mode", list(RECORDS))
def test_corrections_gain_a_permutation_test_against_raw(mode, kind):
    m = _model()
    t, v, tm, vm, cut = _sets()[kind]
    record = RECORDS[mode]()
    n_units = v.shape[0]

    def run(a, **kw):
        return evaluator.sharded_evaluation(m, t, v, tm, vm, a, record, cut_off_points=cut, **kw)
    plain = run(ARGS, ir=True)
    off = run(ARGS, ir=True, permutation=0, permutation_seed=5)
    on = run(ARGS, ir=True, **PERM)
    bare = run(ARGS, **PERM)
    for d in range(2):
        assert _same_tree(off[d], plain[d])                                         # permutation = 0: today's keys and values
        raw, cor = on[d], on[d][record.key]
        # nothing but the new entries: "units" and the IR "columns" everywhere, "permutation_vs_raw" in the correction
        strip = dict(_without(raw, "units", record.key), ir=_without(raw["ir"], "columns"))
        strip[record.key] = dict(_without(cor, "units", "permutation_vs_raw"), ir=_without(cor["ir"], "columns", "permutation_vs_raw"))
        assert _same_tree(strip, plain[d])
        assert "permutation_vs_raw" not in raw and "permutation_vs_raw" not in raw["ir"]
        for x in (raw, cor):
            assert set(x["units"]) == {"entries", "unit_end", "median"} and len(x["units"]["unit_end"]) == n_units
            assert x["units"]["median"] == ("low" if kind == "multi" and d == 0 else "mid")
            assert x["ir"]["columns"].shape == (n_units, 5) and x["ir"]["columns"].dtype == np.int64
        if "cols" in raw:
            assert raw["units"]["entries"].tolist() == raw["cols"] and cor["units"]["entries"].tolist() == cor["cols"]
        # the summaries are the restatement's, run on the carried units: seed for text->video, seed + 1 for video->text
        assert cor["permutation_vs_raw"] == _want_rank_summary(cor["units"], raw["units"], SEED + d)
        assert cor["ir"]["permutation_vs_raw"] == _want_ir_summary(cor["ir"]["columns"], raw["ir"]["columns"], SEED + d)
        for key in ("R1", "MeanR"):                  # the multi-sentence text->video dictionary rounds its figures to float32 (6.7)
            slack = 2.0 ** -23 * (abs(cor[key]) + abs(raw[key])) if kind == "multi" and d == 0 else 1e-12
            assert cor["permutation_vs_raw"][key]["diff"] == pytest.approx(cor[key] - raw[key], rel=0, abs=slack)
        assert cor["ir"]["permutation_vs_raw"]["MRR"]["diff"] == pytest.approx(cor["ir"]["MRR"] - raw["ir"]["MRR"], rel=1e-9, abs=1e-9)
        # without --ir_metrics there is no IR entry to extend
        assert "ir" not in bare[d] and "ir" not in bare[d][record.key]
        assert _same_tree(bare[d][record.key]["permutation_vs_raw"], cor["permutation_vs_raw"])
    for out in _emulated(3, lambda a, r: run(a, ir=True, **PERM)):                   # three ranks: the same trees on every rank
        for d in range(2):
            assert _same_tree(out[d], on[d])


def test_raw_evaluation_carries_its_units_and_the_legacy_entry_points_forward_the_arguments():
    m = _model()
    t, v, tm, vm, cut = _sets()["multi"]
    s = _sets()["single"][:4]
    raw = evaluator.sharded_evaluation(m, t, v, tm, vm, ARGS, cut_off_points=cut, ir=True, **PERM)
    plain = evaluator.sharded_evaluation(m, t, v, tm, vm, ARGS, cut_off_points=cut, ir=True)
    for d in range(2):
        assert _same_tree(dict(_without(raw[d], "units"), ir=_without(raw[d]["ir"], "columns")), plain[d])
    legacy = evaluator.sharded_multi_sentence_metrics(m, t, v, tm, vm, cut, ARGS, ir=True, **PERM)
    hub = evaluator.sharded_metrics_with_hubness(m, t, v, tm, vm, ARGS, 3, cut_off_points=cut, ir=True, **PERM)
    for d in range(2):
        assert _same_tree(legacy[d], raw[d]) and _same_tree(_without(hub[d], "hubness"), raw[d])
    want = evaluator.sharded_evaluation(m, *s, ARGS, ir=True, **PERM)
    got = evaluator.sharded_metrics(m, *s, ARGS, ir=True, **PERM)
    for d in range(2):
        assert _same_tree(got[d], want[d]) and "units" in got[d]
    for fn, mode, record in ((evaluator.sharded_metrics_with_test_norm, "dsl", evaluator.test_norm_correction("dsl")),
                             (evaluator.sharded_metrics_with_local_scaling, "csls", evaluator.local_scaling_correction("csls")),
                             (evaluator.sharded_metrics_with_mutual_proximity, "emp", evaluator.mutual_proximity_correction("emp"))):
        got = fn(m, *s, ARGS, mode, **PERM)
        want = evaluator.sharded_evaluation(m, *s, ARGS, record, **PERM)
        for d in range(2):
            assert _same_tree(got[d], want[d]) and "permutation_vs_raw" in got[d][record.key]


# ---- comparing two evaluations ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _perturbed_model():
    """A copy of the model whose weight matrices moved by a tenth of their spread: another checkpoint of the same architecture."""
    other = copy.deepcopy(_model())
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in other.parameters():
            if p.dim() >= 2:
                p.add_((0.1 * p.std().cpu() * torch.randn(p.shape, generator=gen)).to(p.device))
    return other


def test_compare_evaluations_of_two_models_equals_the_restatement():
    t, v, tm, vm, cut = _sets()["multi"]
    record = evaluator.test_norm_correction("dsl", 12.5)

    def run(model, **kw):
        return evaluator.sharded_evaluation(model, t, v, tm, vm, ARGS, record, cut_off_points=cut, **{**PERM, "ir": True, **kw})
    a, b = run(_model()), run(_perturbed_model())
    assert any(not np.array_equal(a[d]["units"]["entries"], b[d]["units"]["entries"]) for d in range(2))     # the copy ranks otherwise
    cmp = evaluator.compare_evaluations(a, b, NP, SEED, bootstrap=16, bootstrap_seed=3, bootstrap_level=0.9, device=DEV)
    assert len(cmp) == 2
    for d in range(2):
        assert set(cmp[d]) == {"permutation", "bootstrap", "ir", "test_norm"}
        for got, x, y in ((cmp[d], a[d], b[d]), (cmp[d]["test_norm"], a[d]["test_norm"], b[d]["test_norm"])):
            assert set(got) >= {"permutation", "bootstrap", "ir"} and set(got["ir"]) == {"permutation", "bootstrap"}
            assert got["permutation"] == _want_rank_summary(x["units"], y["units"], SEED + d)
            assert got["ir"]["permutation"] == _want_ir_summary(x["ir"]["columns"], y["ir"]["columns"], SEED + d)
            # the paired bootstrap: the existing summaries on the draws of the bootstrap (seed 3, then 4)
            ux, uy = x["units"], y["units"]
            stats = ops.bootstrap_rank_stats(_i32(ux["entries"]), _i32(ux["unit_end"]), _i32(uy["entries"]), _i32(uy["unit_end"]),
                                             seed=3 + d, n_boot=16).cpu().numpy()
            want = RetrievalMetrics.paired_bootstrap_summary(stats[:, 0], stats[:, 1], CUTS, ux["entries"], uy["entries"], 0.9, ux["median"])
            assert _same_tree(got["bootstrap"], dict(want, seed=3 + d))
            sums = ops.bootstrap_unit_sums(_i64(np.concatenate([x["ir"]["columns"], y["ir"]["columns"]], axis=1)), seed=3 + d, n_boot=16)
            want = RetrievalMetrics.ir_paired_bootstrap_summary(sums, x["ir"]["columns"], y["ir"]["columns"], 0.9)
            assert _same_tree(got["ir"]["bootstrap"], dict(want, seed=3 + d))
    # without the bootstrap and without IR on one side: only what both carry is compared
    lean = evaluator.compare_evaluations(a, run(_perturbed_model(), ir=False), NP, SEED, device=DEV)
    for d in range(2):
        assert set(lean[d]) == {"permutation", "test_norm"} and set(lean[d]["test_norm"]) == {"permutation"}
        assert lean[d]["permutation"] == cmp[d]["permutation"]
    # b minus a: the differences change sign, the one-sided p-values change places
    back = evaluator.compare_evaluations(b, a, NP, SEED, device=DEV)
    for d in range(2):
        for key in ("R1", "R5", "MeanR", "MedianR"):
            x, y = cmp[d]["permutation"][key], back[d]["permutation"][key]
            assert y == dict(diff=-x["diff"], p_two=x["p_two"], p_ge=x["p_le"], p_le=x["p_ge"])


def test_a_model_against_itself_and_mismatched_sets():
    m = _model()
    t, v, tm, vm, _ = _sets()["single"]
    a = evaluator.sharded_evaluation(m, t, v, tm, vm, ARGS, ir=True, **PERM)
    again = evaluator.sharded_evaluation(m, t, v, tm, vm, ARGS, ir=True, **PERM)
    cmp = evaluator.compare_evaluations(a, again, NP, SEED, bootstrap=8, device=DEV)
    for d in range(2):
        assert (cmp[d]["permutation"]["n_perm"], cmp[d]["permutation"]["kept"], cmp[d]["permutation"]["seed"]) == (NP, NP, SEED + d)
        for key in ("R1", "R5", "R10", "R50", "MedianR", "MeanR"):
            assert cmp[d]["permutation"][key] == dict(diff=0.0, p_two=1.0, p_ge=1.0, p_le=1.0), key
            assert cmp[d]["bootstrap"][key]["point"] == 0.0 and cmp[d]["bootstrap"][key]["se"] == 0.0
        for key in RetrievalMetrics.IR_METRICS:
            assert cmp[d]["ir"]["permutation"][key] == dict(diff=0.0, p_two=1.0, p_ge=1.0, p_le=1.0), key
    fewer = evaluator.sharded_evaluation(m, t[:20], v[:20], tm[:20], vm[:20], ARGS, ir=True, **PERM)
    with pytest.raises(ValueError, match="24 and 20 units"):
        evaluator.compare_evaluations(a, fewer, NP, device=DEV)
    mt, mv, mtm, mvm, cut = _sets()["multi"]
    multi = evaluator.sharded_evaluation(m, mt, mv, mtm, mvm, ARGS, cut_off_points=cut, **PERM)
    nine = evaluator.sharded_evaluation(m, t[:9], v[:9], tm[:9], vm[:9], ARGS, **PERM)
    with pytest.raises(ValueError, match="different medians"):                       # 9 units each, but videos against queries
        evaluator.compare_evaluations(multi, nine, NP, device=DEV)
    with pytest.raises(ValueError, match="carries no units"):
        evaluator.compare_evaluations(a, evaluator.sharded_evaluation(m, t, v, tm, vm, ARGS), NP, device=DEV)


def test_a_querybank_correction_gains_the_entries_too():
    m = _model()
    t, v, tm, vm, _ = _sets()["single"]
    on = evaluator.sharded_evaluation(m, t, v, tm, vm, ARGS, evaluator.test_norm_correction("qbnorm", 12.5, 2), querybank=_bank(), **PERM)
    for d in range(2):
        assert on[d]["test_norm"]["permutation_vs_raw"] == _want_rank_summary(on[d]["test_norm"]["units"], on[d]["units"], SEED + d)


# ---- the two eval_epoch callers ------------------------------------------------------------------------------------------------------------
class Loader:
    def __init__(self, batches):
        self.batches, self.dataset = batches, None

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def test_training_eval_epoch_logs_the_permutation_test(caplog):
    t, v, tm, vm = (x.cpu() for x in _testset())
    batches = [(t[ix], tm[ix].long(), v[ix], vm[ix].long(), ix.clone(), ix.clone())
               for ix in (torch.arange(lo, min(lo + 32, N)) for lo in range(0, N, 32))]
    args = SimpleNamespace(world_size=1, rank=0, local_rank=0, logger=logging.getLogger("test_permtest"), test_norm="dsl",
                           ir_metrics=1, permutation=NP, permutation_seed=SEED)
    with caplog.at_level(logging.INFO, logger="test_permtest"):
        on = training.eval_epoch(args, _model(), Loader(batches), torch.device(DEV))
    lines = [r.getMessage() for r in caplog.records]
    want = evaluator.sharded_evaluation(_model(), *_testset(), ARGS, evaluator.test_norm_correction("dsl"), ir=True, **PERM)
    for d, side in enumerate(("Text-to-Video", "Video-to-Text")):
        assert _same_tree(on[d], want[d])
        cor = on[d]["test_norm"]
        assert RetrievalMetrics.format_permutation(cor["permutation_vs_raw"], prefix=f"{side} [DSL b=20] - raw: ") in lines
        assert RetrievalMetrics.format_permutation(cor["ir"]["permutation_vs_raw"], prefix=f"{side} [DSL b=20] - raw: ") in lines
    assert sum("permutation" in line for line in lines) == 4


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def _run_main(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--synthetic_test", "64"]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()]


def test_main_retrieval_logs_the_permutation_test_of_a_correction():
    lines = _run_main("--test_norm", "dsl", "--ir_metrics", "1", "--permutation", "200", "--permutation_seed", "3")
    perm = [line for line in lines if "permutation" in line]
    assert len(perm) == 4, lines
    at = lines.index(perm[0])
    assert lines[at - 1].startswith("video->text [DSL b=20]: MRR ") and lines[at + 1] == perm[1]      # after the correction's IR lines
    assert perm[0].startswith("text->video [DSL b=20] - raw R@1: ") and perm[1].startswith("text->video [DSL b=20] - raw MRR: ")
    assert perm[2].startswith("video->text [DSL b=20] - raw R@1: ") and perm[3].startswith("video->text [DSL b=20] - raw MRR: ")
    for line in perm:
        assert line.endswith("(paired permutation test vs raw, 200 permutations)") and " p=" in line
    assert "Median R: " in perm[0] and "Mean R: " in perm[0] and "R-Prec: " in perm[1]


def test_main_retrieval_compares_with_a_second_checkpoint(tmp_path, monkeypatch):
    """The checkpoint: the command line's own model (its seed, its architecture) with every weight matrix moved."""
    sys.path.insert(0, ROOT)
    import main_retrieval
    from neighborretr_amd.modeling import NeighborRetr
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py", "--do_eval", "1", "--synthetic"])
    args = main_retrieval.get_args()
    torch.manual_seed(args.seed)                                                 # main() seeds torch, then builds the model
    state = NeighborRetr(args, precision=args.precision, with_encoders=False).state_dict()
    gen = torch.Generator().manual_seed(9)
    for name, p in state.items():
        if p.dim() >= 2 and p.is_floating_point():
            state[name] = p + 0.1 * p.std() * torch.randn(p.shape, generator=gen)
    path = os.path.join(str(tmp_path), "other.bin")
    torch.save(state, path)
    lines = _run_main("--permutation", "128", "--bootstrap", "50", "--compare_model", path)
    assert f"compare_model {path}: 0 missing / 0 unexpected keys" in lines
    metrics = [line for line in lines if line.startswith("text->video R@1 ")]
    assert len(metrics) == 2 and metrics[0] != metrics[1]                           # the model, then the compared one: another ranking
    cmp = [line for line in lines if line.startswith("model - compared ")]
    assert len(cmp) == 4 and lines[-4:] == cmp, lines
    for line, side in zip(cmp[::2], ("text->video", "video->text")):
        assert line.startswith(f"model - compared {side} R@1: ") and line.endswith("(paired permutation test vs compared, 128 permutations)")
    for line, side in zip(cmp[1::2], ("text->video", "video->text")):
        assert line.startswith(f"model - compared {side} R@1: ") and "frac<=0" in line
        assert line.endswith("(95% paired bootstrap vs compared, 50 resamples)")
