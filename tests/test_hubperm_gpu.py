"""GPU: nr_permtest_hubness against its restatement (hubperm_ref) integer for integer at the shapes where it can go wrong, above 64 KB
of LDS, under any split over p0 and against nr_permtest_unit_sums' swap bits; the wrapper's refusals; the evaluator's hubness_test
entries against the restatement, under emulated ranks and in compare_evaluations; the log lines of the two eval_epoch callers."""
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hubperm_ref as H
from neighborretr_amd import evaluator, hip, ops, training
from neighborretr_amd.metrics import RetrievalMetrics
from test_evaldriver_gpu import _sets
from test_irmetrics_gpu import DEV, N, _emulated, _model, _same_tree, _testset, _without
from test_permtest_gpu import Loader, _perturbed_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = RetrievalMetrics.HUBNESS_TEST_METRICS


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _gpu(case, **kw):
    a, b, unit_end, G, gb, ge = case
    out = ops.permtest_hubness(_i32(a), _i32(b), _i32(unit_end), G, _i32(gb), _i32(ge), **kw)
    assert out.dtype == torch.int64 and out.is_cuda and out.shape[1:] == (2, 9)
    return out.cpu().numpy()


def _ref(case, **kw):
    return H.hubness_stats(*case, **kw)


def _lists(rng, n_lists, k, G, weight=1.0, absent=0.05, outside=0.03):
    """Top-k lists (distinct items, the most popular first) padded with -1 where G < k; some slots absent, some indices outside."""
    pop = np.linspace(3.0, 0.0, G)
    order = np.argsort(-(weight * pop[None, :] + rng.standard_normal((n_lists, G))), axis=1, kind="stable")[:, :k]
    idx = np.full((n_lists, k), -1, dtype=np.int32)
    idx[:, :order.shape[1]] = order
    idx[rng.random(idx.shape) < absent] = -1
    out = rng.random(idx.shape) < outside
    idx[out] = np.where(rng.random(int(out.sum())) < 0.5, G, G + 70000)
    return idx


def _case(rng, U, k, G, sizes=None, gt_width=1):
    """(idx_a, idx_b, unit_end, G, gt_begin, gt_end): U units of one list each, or of `sizes` lists."""
    sizes = np.ones(U, dtype=np.int64) if sizes is None else np.asarray(sizes)
    n_lists = int(sizes.sum())
    gb = rng.integers(0, G, n_lists)
    return _lists(rng, n_lists, k, G, 2.0), _lists(rng, n_lists, k, G, 0.3), np.cumsum(sizes) - 1, G, gb, gb + gt_width


# ---- the kernel against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 15, 128])
@pytest.mark.parametrize("U", [1, 2, 63, 64, 257])
def test_kernel_equals_the_restatement_integer_for_integer(U, k):
    rng = np.random.default_rng(1000 * U + k)
    for G in (1, 2, 100, 1000):                                                  # G < k: the lists are padded
        case = _case(rng, U, k, G)
        n_perm = 6 if U * k < 5000 else 3
        got, want = _gpu(case, seed=7, p0=2, n_perm=n_perm), _ref(case, seed=7, p0=2, n_perm=n_perm)
        assert np.array_equal(got, want), (G, got[0].tolist(), want[0].tolist())
        ma, mb = (H.moments(*H.counts(x.tolist(), G, case[4], case[5])) for x in case[:2])
        assert np.array_equal((got[:, 0] + got[:, 1])[:, [0, 7]], np.tile([ma[0] + mb[0], ma[7] + mb[7]], (n_perm, 1)))


def _special_cases():
    rng = np.random.default_rng(77)
    cases = {}
    a, b, end, G, gb, ge = _case(rng, 20, 5, 50)
    a[3] = -1                                                                    # a list that is all absent
    b[3, 1:] = -1
    cases["a_list_all_absent"] = (a, b, end, G, gb, ge)
    a, b, end, G, gb, ge = _case(rng, 2, 3, 10)
    cases["an_empty_side"] = (np.full_like(a, -1), b, end, G, gb, ge)            # X is empty whenever both units come from A
    sizes = rng.integers(0, 7, 40)
    sizes[[0, 5, 6, 39]] = 0
    sizes[17] += 130 - sizes.sum()
    assert sizes.sum() == 130 and sizes.min() == 0
    cases["130_lists_in_40_units"] = _case(rng, 40, 15, 100, sizes=sizes, gt_width=3)
    a, _, end, G, gb, ge = _case(rng, 64, 15, 100)
    cases["a_equals_b"] = (a, a.copy(), end, G, gb, ge)
    one = np.full((257, 3), -1, dtype=np.int32)
    one[:, 0] = 41                                                               # every list of A on one item: N = 257 there
    uniform = np.stack([(3 * q + np.arange(3)) % 100 for q in range(257)]).astype(np.int32)
    cases["one_item_against_uniform"] = (one, uniform, np.arange(257), 100, np.full(257, 41), np.full(257, 42))
    # a multi-sentence set, text->video: 9 videos own 1-6 sentences each, a sentence's ground truth is its video ...
    sizes = np.asarray([1, 6, 2, 1, 5, 3, 4, 1, 2])
    video = np.repeat(np.arange(9), sizes)
    cases["multi_sentence_rows"] = (_lists(rng, 25, 5, 9, 2.0), _lists(rng, 25, 5, 9, 0.0), np.cumsum(sizes) - 1, 9, video, video + 1)
    # ... and video->text: one list per video over the 25 sentences, its ground truth its group's range
    ends = np.cumsum(sizes)
    cases["multi_sentence_columns"] = (_lists(rng, 9, 5, 25, 2.0), _lists(rng, 9, 5, 25, 0.0), np.arange(9), 25, ends - sizes, ends)
    return cases


SPECIAL = _special_cases()


@pytest.mark.parametrize("name", list(SPECIAL))
def test_special_cases_equal_the_restatement(name):
    case = SPECIAL[name]
    got, want = _gpu(case, seed=3, n_perm=40), _ref(case, seed=3, n_perm=40)
    assert np.array_equal(got, want)
    if name == "an_empty_side":
        assert (got[:, 0, 0] == 0).any() and (got[:, 1, 0] == 0).any() and (got[:, :, 0] > 0).all(axis=1).any()
        empty = got[got[:, 0, 0] == 0][0, 0]
        assert empty.tolist() == [0, 0, 0, 10, 0, 0, 0, 0, 0]                    # an empty side: every item an anti-hub, no hub
        ma, mb = (H.moments(*H.counts(x.tolist(), 10, case[4], case[5])) for x in case[:2])
        s = RetrievalMetrics.hubness_permutation_summary(got, mb, mb, 10, seed=3)
        assert s["n_empty"] == int(((got[:, 0, 0] == 0) | (got[:, 1, 0] == 0)).sum()) > 0 and s["kept"] == 40 - s["n_empty"]
        assert ma[0] == 0 and np.isnan(RetrievalMetrics.hubness_permutation_summary(got, ma, mb, 10)["skewness"]["p_two"])
    if name == "a_equals_b":
        ma = H.moments(*H.counts(case[0].tolist(), case[3], case[4], case[5]))
        assert all(side == ma for row in got.tolist() for side in row)
    if name == "one_item_against_uniform":
        assert got[:, :, 8].max() > 100 and got[:, :, 4].min() >= 1              # item 41 is a hub on both sides of every relabelling


@pytest.mark.parametrize("G", [20000, 32768])
def test_galleries_whose_counters_need_more_than_64_kb_of_lds(G):
    assert 4 * G + 576 > 64 * 1024
    rng = np.random.default_rng(G)
    gb = rng.integers(0, G, 64)
    a = rng.integers(0, G, (64, 3)).astype(np.int32)
    a[:, 0], a[:, 1] = G - 1, np.arange(64) * (G // 64)                          # the last counter, and counters all over the LDS
    b = rng.integers(0, G, (64, 3)).astype(np.int32)
    b[:, 0], b[:, 2] = np.arange(64), G                                          # the first counters; the first index outside
    case = (a, b, np.arange(64), G, gb, gb + 2)
    assert np.array_equal(_gpu(case, seed=1, n_perm=4), _ref(case, seed=1, n_perm=4))


def test_limits_are_refused_with_the_limit_in_the_message():
    z = _i32(np.zeros((4, 3)))
    e, g = _i32(np.arange(4)), _i32(np.arange(4))
    with pytest.raises(ValueError, match="32769 is above the 32768 items"):
        ops.permtest_hubness(z, z, e, 32769, g, g, n_perm=2)
    many = torch.zeros((65536, 1), dtype=torch.int32, device=DEV)
    ends, gt = torch.arange(65536, dtype=torch.int32, device=DEV), torch.zeros(65536, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="65536 lists are above the limit of 65535"):
        ops.permtest_hubness(many, many, ends, 10, gt, gt, n_perm=2)
    assert ops.permtest_hubness(many[:65535], many[:65535], ends[:65535], 10, gt[:65535], gt[:65535], n_perm=1).shape == (1, 2, 9)
    # the entry point itself answers NR_EUNSUPPORTED (-2)
    with pytest.raises(hip.NrHipError, match="status -2"):
        hip.call("nr_permtest_hubness", hip.ptr(z), hip.ptr(z), 4, 3, hip.ptr(e), 4, 32769, hip.ptr(g), hip.ptr(g), hip.ptr(g), hip.ptr(g),
                 0, 0, 2, hip.ptr(torch.zeros(36, dtype=torch.int64, device=DEV)), hip.stream_ptr())


def test_any_split_over_p0_a_late_p0_and_a_large_seed_give_the_same_integers():
    rng = np.random.default_rng(5)
    case = _case(rng, 70, 7, 60, sizes=rng.integers(0, 4, 70))
    whole = _gpu(case, seed=9, p0=0, n_perm=50)
    assert np.array_equal(whole, _ref(case, seed=9, n_perm=50))
    for cut in (1, 17, 49):
        parts = np.concatenate([_gpu(case, seed=9, p0=0, n_perm=cut), _gpu(case, seed=9, p0=cut, n_perm=50 - cut)])
        assert np.array_equal(parts, whole)
    assert _gpu(case, seed=9, p0=3, n_perm=0).shape == (0, 2, 9)
    late, seed = (1 << 31) - 4, (1 << 64) - 2
    assert np.array_equal(_gpu(case, seed=seed, p0=late, n_perm=3), _ref(case, seed=seed, p0=late, n_perm=3))
    assert not np.array_equal(_gpu(case, seed=10, n_perm=50), whole)


@pytest.mark.parametrize("U", [1, 2, 63, 64, 257, 1000])
def test_swap_bits_are_those_of_the_unit_sums_kernel(U):
    """Every list of A is [0], every list of B is [1], every ground truth is item 0: side X's good occurrences are N_X[0], the units
    with s = 0 -- the unit-sum of a column of ones against a column of zeros."""
    zeros, ones = np.zeros((U, 1), dtype=np.int32), np.ones((U, 1), dtype=np.int32)
    case = (zeros, ones, np.arange(U), 2, np.zeros(U), np.ones(U))
    seed, p0, n_perm = 1234, 3, 128
    got = _gpu(case, seed=seed, p0=p0, n_perm=n_perm)
    col = lambda x: torch.from_numpy(x.astype(np.int64)).to(DEV)
    sums = ops.permtest_unit_sums(col(ones), col(zeros), seed=seed, p0=p0, n_perm=n_perm).cpu().numpy()[:, 0]
    assert np.array_equal(got[:, 0, 7], sums) and np.array_equal(got[:, 1, 7], U - sums)
    assert np.array_equal(got[:, 0, 0], np.full(n_perm, U)) and np.array_equal(got[:, 0, 1], sums ** 2 + (U - sums) ** 2)
    if U >= 63:
        assert 0 < sums.min() and sums.max() < U and len(set(sums.tolist())) > 3


def test_wrapper_refuses_bad_arguments():
    a = _i32(np.arange(12).reshape(4, 3))
    e, g = _i32([0, 1, 3]), _i32(np.arange(4))
    good = dict(idx_a=a, idx_b=a, unit_end=e, n_gallery=20, gt_begin=g, gt_end=g + 1, n_perm=2)
    assert ops.permtest_hubness(**good).shape == (2, 2, 9) and ops.permtest_hubness(**dict(good, n_perm=0)).shape == (0, 2, 9)
    wide = torch.zeros((4, 129), dtype=torch.int32, device=DEV)
    bad = [dict(idx_a=a.long()), dict(idx_b=a.cpu()), dict(idx_a=a[0]), dict(idx_b=a[:3]), dict(idx_b=a[:, :2]), dict(idx_a=None),
           dict(idx_a=wide, idx_b=wide), dict(idx_a=a[:, :0], idx_b=a[:, :0]),                               # k outside [1, 128]
           dict(unit_end=e.cpu()), dict(unit_end=e.float()), dict(unit_end=_i32([])), dict(unit_end=_i32([[0, 1, 3]])),
           dict(unit_end=_i32([1, 0, 3])), dict(unit_end=_i32([0, 1, 2])), dict(unit_end=_i32([0, 1, 4])), dict(unit_end=_i32([-2, 1, 3])),
           dict(gt_begin=g[:3]), dict(gt_end=g.long()), dict(gt_begin=g.cpu()), dict(gt_end=None),
           dict(n_gallery=0), dict(n_gallery=-3), dict(n_gallery=2.5), dict(n_gallery=32769), dict(n_gallery=True),
           dict(p0=-1), dict(n_perm=-1), dict(p0=(1 << 31) - 2, n_perm=2), dict(seed=-1), dict(seed=1 << 64), dict(n_perm=2.5)]
    for over in bad:
        with pytest.raises(ValueError):
            ops.permtest_hubness(**dict(good, **over))
    # the entry point's own refusal surfaces through hip.call (NR_EINVAL = -1): k = 0
    out = torch.zeros(36, dtype=torch.int64, device=DEV)
    with pytest.raises(hip.NrHipError, match="status -1"):
        hip.call("nr_permtest_hubness", hip.ptr(a), hip.ptr(a), 4, 0, hip.ptr(e), 3, 20, hip.ptr(g), hip.ptr(g), hip.ptr(g), hip.ptr(g), 0, 0,
                 2, hip.ptr(out), hip.stream_ptr())


# ---- the sharded evaluator ------------------------------------------------------------------------------------------------------------
NP, SEED, K = 64, 11, 5
PERM = dict(permutation=NP, permutation_seed=SEED)
TEST = dict(PERM, hubness_k=K, hubness_test=True)
ARGS = SimpleNamespace(world_size=1)


def _want_summary(hub, other, seed):
    la, lb = hub["lists"], other["lists"]
    G = hub["n_gallery"]
    stats = H.hubness_stats(la["idx"], lb["idx"], la["unit_end"], G, la["gt_begin"], la["gt_end"], seed=seed, n_perm=NP)
    moments = (H.moments(h["occurrence"].tolist(), h["good_occurrence"].tolist()) for h in (hub, other))
    return H.summary(stats, *moments, G, seed=seed)


@pytest.mark.parametrize("kind", ["single", "multi"])
def test_a_correction_gains_a_hubness_test_against_raw(kind):
    m = _model()
    t, v, tm, vm, cut = _sets()[kind]
    record = evaluator.test_norm_correction("dsl", 12.5)
    n_rows, n_cols = t.shape[0], v.shape[0]

    def run(a, **kw):
        return evaluator.sharded_evaluation(m, t, v, tm, vm, a, record, cut_off_points=cut, **kw)
    plain = run(ARGS, hubness_k=K, **PERM)
    off = run(ARGS, hubness_k=K, hubness_test=False, **PERM)
    on = run(ARGS, **TEST)
    for d in range(2):
        assert _same_tree(off[d], plain[d])                                      # without the flag: today's keys and values
        raw, cor = on[d], on[d][record.key]
        strip = dict(_without(raw, record.key), hubness=_without(raw["hubness"], "lists"))
        strip[record.key] = dict(cor, hubness=_without(cor["hubness"], "lists", "permutation_vs_raw"))
        assert _same_tree(strip, plain[d])                                       # nothing but the new entries
        assert "permutation_vs_raw" not in raw["hubness"]
        n_lists, G = (n_rows, n_cols) if d == 0 else (n_cols, n_rows)
        for x in (raw, cor):
            lists = x["hubness"]["lists"]
            assert set(lists) == {"idx", "unit_end", "gt_begin", "gt_end"} and all(isinstance(a, np.ndarray) for a in lists.values())
            assert lists["idx"].shape == (n_lists, K) and lists["idx"].dtype == np.int32 and x["hubness"]["n_gallery"] == G
            assert len(lists["unit_end"]) == n_cols and lists["unit_end"][-1] == n_lists - 1      # the unit: the query, or the video
            assert H.counts(lists["idx"].tolist(), G, lists["gt_begin"], lists["gt_end"]) == \
                (x["hubness"]["occurrence"].tolist(), x["hubness"]["good_occurrence"].tolist())
        got = cor["hubness"]["permutation_vs_raw"]
        assert got == _want_summary(cor["hubness"], raw["hubness"], SEED + d)    # seed for text->video, seed + 1 for video->text
        assert (got["n_perm"], got["seed"]) == (NP, SEED + d)
        for name in ("anti_hub_pct", "hub_pct", "bad_hub_pct", "hub_occurrence_pct", "good_occurrence_pct", "max_occurrence"):
            assert got[name]["diff"] == pytest.approx(cor["hubness"][name] - raw["hubness"][name], rel=0, abs=1e-9)
        assert got["skewness"]["diff"] == pytest.approx(cor["hubness"]["skewness"] - raw["hubness"]["skewness"], rel=0, abs=1e-9)
    for out in _emulated(2, lambda a, r: run(a, **TEST)):                        # two ranks: the same trees on every rank
        for d in range(2):
            assert _same_tree(out[d], on[d])


def test_hubness_test_needs_its_two_flags_before_any_scoring():
    t, v, tm, vm, _ = _sets()["single"]
    for kw in (dict(PERM, hubness_test=True), dict(hubness_k=K, hubness_test=True)):
        with pytest.raises(ValueError, match="hubness_test needs hubness_k > 0 .* and permutation > 0"):
            evaluator.sharded_evaluation(None, t, v, tm, vm, ARGS, **kw)         # no model: nothing may be scored


def test_compare_evaluations_of_two_models_and_of_a_model_with_itself():
    t, v, tm, vm, cut = _sets()["multi"]
    record = evaluator.test_norm_correction("dsl", 12.5)

    def run(model, **kw):
        return evaluator.sharded_evaluation(model, t, v, tm, vm, ARGS, record, cut_off_points=cut, **{**TEST, **kw})
    a, b = run(_model()), run(_perturbed_model())
    assert any(not np.array_equal(a[d]["hubness"]["lists"]["idx"], b[d]["hubness"]["lists"]["idx"]) for d in range(2))
    cmp = evaluator.compare_evaluations(a, b, NP, SEED, device=DEV)
    for d in range(2):
        for got, x, y in ((cmp[d], a[d], b[d]), (cmp[d]["test_norm"], a[d]["test_norm"], b[d]["test_norm"])):
            assert set(got["hubness"]) == {"k", "permutation"} and got["hubness"]["k"] == K
            assert got["hubness"]["permutation"] == _want_summary(x["hubness"], y["hubness"], SEED + d)
    # only what both carry is compared
    lean = evaluator.compare_evaluations(a, run(_perturbed_model(), hubness_test=False), NP, SEED, device=DEV)
    assert all("hubness" not in lean[d] and "hubness" not in lean[d]["test_norm"] for d in range(2))
    same = evaluator.compare_evaluations(a, run(_model()), NP, SEED, device=DEV)
    for d in range(2):
        s = same[d]["hubness"]["permutation"]
        assert (s["n_perm"], s["kept"], s["seed"]) == (NP, NP, SEED + d)
        for name in FIGURES:
            assert s[name] == dict(diff=0.0, p_two=1.0, p_ge=1.0, p_le=1.0), name
    with pytest.raises(ValueError, match=r"\(k = 5\) and .* \(k = 3\)"):
        evaluator.compare_evaluations(a, run(_model(), hubness_k=3), NP, device=DEV)
    # another gallery over as many units: the first 9 items of the single-sentence set against the 9 videos' 31 sentences
    st, sv, stm, svm, _ = _sets()["single"]
    n = v.shape[0]
    small = evaluator.sharded_evaluation(_model(), st[:n], sv[:n], stm[:n], svm[:n], ARGS, **TEST)
    multi = evaluator.sharded_evaluation(_model(), t, v, tm, vm, ARGS, cut_off_points=cut, **TEST)
    small = tuple(dict(x, units=y["units"]) for x, y in zip(small, multi))      # the rank units pair up; the lists do not
    with pytest.raises(ValueError, match="top-k lists are|galleries hold"):
        evaluator.compare_evaluations(multi, small, NP, device=DEV)


# ---- the two eval_epoch callers ---------------------------------------------------------------------------------------------------------
def test_training_eval_epoch_logs_the_hubness_test(caplog):
    t, v, tm, vm = (x.cpu() for x in _testset())
    batches = [(t[ix], tm[ix].long(), v[ix], vm[ix].long(), ix.clone(), ix.clone())
               for ix in (torch.arange(lo, min(lo + 32, N)) for lo in range(0, N, 32))]
    args = SimpleNamespace(world_size=1, rank=0, local_rank=0, logger=logging.getLogger("test_hubperm"), test_norm="dsl", hubness_k=K,
                           hubness_test=1, permutation=NP, permutation_seed=SEED)
    with caplog.at_level(logging.INFO, logger="test_hubperm"):
        on = training.eval_epoch(args, _model(), Loader(batches), torch.device(DEV))
    lines = [r.getMessage() for r in caplog.records]
    want = evaluator.sharded_evaluation(_model(), *_testset(), ARGS, evaluator.test_norm_correction("dsl"), **TEST)
    for d, side in enumerate(("Text-to-Video", "Video-to-Text")):
        assert _same_tree(on[d], want[d])
        summary = on[d]["test_norm"]["hubness"]["permutation_vs_raw"]
        line = RetrievalMetrics.format_hubness_permutation(summary, K, prefix=f"{side} [DSL b=20] - raw: ")
        assert line.startswith(f"{side} [DSL b=20] - raw: Hubness@{K}: skew ") and line in lines
        assert lines.index(line) == lines.index(RetrievalMetrics.format_permutation(on[d]["test_norm"]["permutation_vs_raw"],
                                                                                   prefix=f"{side} [DSL b=20] - raw: ")) + 1
    assert sum("permutation test" in line for line in lines) == 4


def test_main_retrieval_logs_the_hubness_test_of_a_correction():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--test_norm", "dsl", "--hubness_k", "5",
           "--permutation", "64", "--hubness_test", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()]
    perm = [line for line in lines if "permutation test" in line]
    assert len(perm) == 4, lines
    for at, side in ((0, "text->video"), (2, "video->text")):
        assert perm[at].startswith(f"{side} [DSL b=20] - raw R@1: ")
        assert perm[at + 1].startswith(f"{side} [DSL b=20] - raw: Hubness@5: skew ") and " - bad hubs " in perm[at + 1]
        assert perm[at + 1].endswith("(paired permutation test vs raw, 64 permutations)") and perm[at + 1].count(" p=") == 7
        assert lines.index(perm[at + 1]) == lines.index(perm[at]) + 1            # next to the existing permutation line
