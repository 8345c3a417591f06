"""GPU: nr_bootstrap_rank_stats against its NumPy restatement (bootstrap_ref) bit for bit, its independence of how the resamples
are split over calls and rankings, the wrapper's refusals, and the bootstrap entries of the sharded evaluator and of both
eval_epoch callers."""
import functools
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bootstrap_ref as B
from neighborretr_amd import evaluator, modeling, ops, synth, training
from neighborretr_amd.metrics import RetrievalMetrics
from util import params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
N, Nt, Nv = 96, 24, 12
CUTS = (1, 5, 10, 50)
WORKED = [[[7, 70012, 3, 3, 2, 6, 6, 6], [5, 2, 0, 0, 4, 5, 5, 5]],
          [[8, 70026, 1, 1, 3, 5, 5, 7], [5, 25, 5, 5, 1, 2, 5, 5]],
          [[6, 70012, 3, 3, 1, 5, 5, 5], [5, 7, 0, 0, 3, 4, 5, 5]]]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _gpu(ranks_a, end_a, ranks_b=None, end_b=None, **kw):
    out = ops.bootstrap_rank_stats(_i32(ranks_a), _i32(end_a), None if ranks_b is None else _i32(ranks_b),
                                   None if end_b is None else _i32(end_b), **kw)
    assert out.dtype == torch.int64 and out.is_cuda
    return out.cpu().numpy()


def _random_ranking(rng, U, high, sizes=(0, 4)):
    """(ranks, unit_end): U units of sizes[0] .. sizes[1] - 1 entries with ranks below `high`."""
    size = rng.integers(sizes[0], sizes[1], U)
    return rng.integers(0, high, int(size.sum())), np.cumsum(size) - 1


# ---- the kernel against the restatement ---------------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(2024)
    c = {}
    c["U1"] = dict(a=([4, 4, 9], [2]), n_boot=3)
    c["U2_one_resample"] = dict(a=([6, 1, 2000], [0, 2]), n_boot=1)
    c["worked_example"] = dict(a=([0, 3, 3, 70000, 1, 0, 12], [0, 2, 2, 3, 6]), b=([0, 0, 5, 2, 9], [0, 1, 2, 3, 4]), seed=42, n_boot=3)
    # more units than threads / not a multiple of them, two rankings of different E, one, two and three digits of the select
    c["U257_small_ranks"] = dict(a=_random_ranking(rng, 257, 1000), b=_random_ranking(rng, 257, 40), seed=5, n_boot=130)
    c["U1000_two_digits"] = dict(a=_random_ranking(rng, 1000, 1 << 20), b=_random_ranking(rng, 1000, 1025), seed=6, n_boot=3)
    c["U1000_three_digits"] = dict(a=_random_ranking(rng, 1000, 1 << 30), b=_random_ranking(rng, 1000, 3), seed=2, n_boot=3)
    c["all_ranks_equal"] = dict(a=(np.full(300, 77), np.arange(300)), b=(np.full(600, 1 << 29), 2 * np.arange(300) + 1), n_boot=3)
    c["every_unit_empty"] = dict(a=([], np.full(9, -1)), b=([5], [-1] * 8 + [0]), n_boot=130)
    c["n_odd"] = dict(a=(rng.integers(0, 30, 5), np.arange(5)), n_boot=130)
    c["n_even_median_between_values"] = dict(a=(np.arange(6) * 1000, np.arange(6)), n_boot=130)
    c["largest_ranks"] = dict(a=([(1 << 30) - 1, 0, (1 << 30) - 1, (1 << 30) - 2, 1 << 20, 1023, 1024], [1, 2, 4, 6]), n_boot=130)
    c["K1"] = dict(a=_random_ranking(rng, 100, 20), cuts=(3,), n_boot=3)
    c["K8"] = dict(a=_random_ranking(rng, 100, 300), b=_random_ranking(rng, 100, 300), cuts=(1, 2, 3, 5, 10, 50, 100, 299), n_boot=3)
    c["large_seed"] = dict(a=_random_ranking(rng, 257, 5000), seed=(1 << 40) + 3, n_boot=3)
    c["largest_seed_late_b0"] = dict(a=_random_ranking(rng, 70, 90), seed=(1 << 64) - 1, b0=(1 << 31) - 4, n_boot=3)
    c["long_units"] = dict(a=_random_ranking(rng, 20, 2000, (0, 90)), b=_random_ranking(rng, 20, 2000, (30, 31)), n_boot=3)
    # the second ranking's select reuses the first one's LDS (hist, wave_tot, pick): both take the successor pass, and a one-pass
    # select follows a three-pass one and the reverse
    c["paired_both_need_the_successor"] = dict(a=(np.arange(6) * 1000, np.arange(6)), b=(np.arange(6) * 1000 + 500, np.arange(6)),
                                               n_boot=130)
    three, one = _random_ranking(rng, 257, 1 << 30), _random_ranking(rng, 257, 40)
    c["paired_one_pass_after_three"] = dict(a=three, b=one, n_boot=130)
    c["paired_three_passes_after_one"] = dict(a=one, b=three, n_boot=130)
    return c


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_restatement_bit_for_bit(name):
    case = dict(CASES[name])
    a, b = case.pop("a"), case.pop("b", (None, None))
    want = B.rank_stats(a[0], a[1], b[0], b[1], **case)
    got = _gpu(a[0], a[1], b[0], b[1], **case)
    assert got.shape == want.shape == (case["n_boot"], 1 if b[0] is None else 2, 4 + len(case.get("cuts", CUTS)))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if name == "worked_example":
        assert got.tolist() == WORKED
    if name == "every_unit_empty":
        assert (got[:, 0] == [0, 0, -1, -1, 0, 0, 0, 0]).all()                        # n = 0: the medians are -1
        assert (got[:, 1, 0] == 0).any() and (got[:, 1, 0] > 0).any()                 # b: only the last unit has an entry
    if name == "n_even_median_between_values":
        assert (got[:, 0, 2] < got[:, 0, 3]).any() and (got[:, 0, 2] == got[:, 0, 3]).any()
    if name == "n_odd":
        assert (got[:, 0, 2] == got[:, 0, 3]).all()
    if name == "paired_both_need_the_successor":
        assert all((got[:, v, 2] < got[:, v, 3]).any() for v in range(2))


def test_any_split_of_the_resamples_and_of_the_rankings_gives_the_same_integers():
    rng = np.random.default_rng(8)
    a, b = _random_ranking(rng, 257, 1 << 12), _random_ranking(rng, 257, 1 << 22)
    whole = _gpu(*a, *b, seed=77, b0=0, n_boot=7)
    parts = [_gpu(*a, *b, seed=77, b0=0, n_boot=3), _gpu(*a, *b, seed=77, b0=3, n_boot=4)]
    assert np.array_equal(whole, np.concatenate(parts))
    assert np.array_equal(whole[:, 0], _gpu(*a, seed=77, n_boot=7)[:, 0])             # V = 2 is two V = 1 calls with the seed
    assert np.array_equal(whole[:, 1], _gpu(*b, seed=77, n_boot=7)[:, 0])
    assert not np.array_equal(whole[:, 0], _gpu(*a, seed=78, n_boot=7)[:, 0])
    assert _gpu(*a, n_boot=0).shape == (0, 1, 8)
    # the default arguments: cuts 1 5 10 50, seed 0, b0 0, 1000 resamples
    assert np.array_equal(_gpu(*a)[:5], B.rank_stats(*a, n_boot=5))


def test_wrapper_refuses_bad_arguments():
    r, e = _i32([0, 3, 2]), _i32([0, 2])
    ok = ops.bootstrap_rank_stats(r, e, n_boot=2)
    assert ok.shape == (2, 1, 8)
    bad = [
        dict(ranks_a=r.long()), dict(ranks_a=r.cpu()), dict(unit_end_a=e.cpu()), dict(unit_end_a=e.float()),   # dtypes and devices
        dict(ranks_a=_i32([0, -1, 2])), dict(ranks_a=_i32([0, 1 << 30, 2])),                                   # ranks outside [0, 2^30)
        dict(unit_end_a=_i32([2, 0])), dict(unit_end_a=_i32([0, 1])), dict(unit_end_a=_i32([0, 3])),           # decreasing / not E - 1
        dict(unit_end_a=_i32([-2, 2])), dict(unit_end_a=_i32([])),
        dict(cuts=(5, 1)), dict(cuts=(1, 1)), dict(cuts=(0, 5)), dict(cuts=()), dict(cuts=tuple(range(1, 10))), dict(cuts=(1.5,)),
        dict(ranks_b=r), dict(unit_end_b=e), dict(ranks_b=r, unit_end_b=_i32([0, 1, 2])),                      # b: both, and U units
        dict(ranks_b=r.cpu(), unit_end_b=e), dict(b0=-1), dict(n_boot=-1), dict(b0=(1 << 31) - 2, n_boot=2), dict(seed=-1),
        dict(seed=1 << 64), dict(n_boot=2.5),
    ]
    for over in bad:
        kw = dict(ranks_a=r, unit_end_a=e, n_boot=2)
        kw.update(over)
        with pytest.raises(ValueError):
            ops.bootstrap_rank_stats(**kw)


# ---- the sharded evaluator ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model():
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _testset(n=N, seed=4242):
    t, v, tm, vm = synth.make_samples(seed, "test", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, v, tm.astype(np.float32), vm.astype(np.float32)))


ARGS = SimpleNamespace(world_size=1)
NB, SEED = 200, 11
BOOT = dict(bootstrap=NB, bootstrap_seed=SEED)
METRICS = ("R1", "R5", "R10", "R50", "MedianR", "MeanR")


def _same_summary(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for key, w in want.items():
        if isinstance(w, np.ndarray):
            assert np.array_equal(got[key], w), key
        else:
            assert got[key] == w, (key, got[key], w)


def _check_direction(metrics, seed, median, n_units, raw=None, point_rel=0.0):
    """One direction's "bootstrap" (and, with the raw direction's dictionary, "bootstrap_vs_raw") against the restatement run on
    the units the summary names, and its points against the dictionary's own figures."""
    boot = metrics["bootstrap"]
    entries, unit_end = boot["entries"], boot["unit_end"]
    assert len(unit_end) == n_units and boot["seed"] == seed and boot["median"] == median
    assert (boot["n_boot"], boot["level"]) == (NB, 0.95)
    if "cols" in metrics:
        assert entries.tolist() == metrics["cols"]                                   # the entries are the ranks the metrics came from
    for key in METRICS:
        assert boot[key]["point"] == pytest.approx(metrics[key], rel=point_rel, abs=0), key
        assert boot[key]["lo"] <= boot[key]["hi"] and boot[key]["se"] >= 0
    if raw is None:
        want = B.rank_stats(entries, unit_end, seed=seed, n_boot=NB)
        assert "bootstrap_vs_raw" not in metrics
    else:
        rb = raw["bootstrap"]
        want = B.rank_stats(entries, unit_end, rb["entries"], rb["unit_end"], seed=seed, n_boot=NB)
        paired = RetrievalMetrics.paired_bootstrap_summary(want[:, 0], want[:, 1], CUTS, entries, rb["entries"], 0.95, median)
        paired["seed"] = seed
        _same_summary(metrics["bootstrap_vs_raw"], paired)
        for key in METRICS:
            assert metrics["bootstrap_vs_raw"][key]["point"] == pytest.approx(metrics[key] - raw[key], rel=point_rel, abs=1e-12)
    summary = RetrievalMetrics.bootstrap_summary(want[:, 0], CUTS, entries, 0.95, median)
    summary.update(seed=seed, entries=entries, unit_end=unit_end)
    _same_summary(boot, summary)


def _without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def test_single_sentence_raw_metrics_gain_a_bootstrap_entry():
    m = _model()
    plain = evaluator.sharded_metrics(m, *_testset(), ARGS)
    on = evaluator.sharded_metrics(m, *_testset(), ARGS, **BOOT)
    off = evaluator.sharded_metrics(m, *_testset(), ARGS, bootstrap=0, bootstrap_seed=5, bootstrap_level=0.5)
    for d in range(2):
        assert off[d] == plain[d] and "bootstrap" not in plain[d]                    # bootstrap = 0: today's keys and values
        assert _without(on[d], "bootstrap") == plain[d]
        _check_direction(on[d], SEED + d, "mid", N)                                  # text->video: seed; video->text: seed + 1
    hub = evaluator.sharded_metrics_with_hubness(m, *_testset(), ARGS, 5, **BOOT)
    for d in range(2):
        _same_summary(hub[d]["bootstrap"], on[d]["bootstrap"])
    level = evaluator.sharded_metrics(m, *_testset(), ARGS, bootstrap=NB, bootstrap_seed=SEED, bootstrap_level=0.5)
    assert level[0]["bootstrap"]["R1"]["se"] == on[0]["bootstrap"]["R1"]["se"]
    assert on[0]["bootstrap"]["MeanR"]["lo"] < level[0]["bootstrap"]["MeanR"]["lo"] < level[0]["bootstrap"]["MeanR"]["hi"] \
        < on[0]["bootstrap"]["MeanR"]["hi"]


@pytest.mark.parametrize("which", ["mutual_proximity", "test_norm", "local_scaling"])
def test_corrections_gain_a_bootstrap_and_a_paired_entry(which):
    m = _model()
    fn, mode = {"mutual_proximity": (evaluator.sharded_metrics_with_mutual_proximity, "emp"),
                "test_norm": (evaluator.sharded_metrics_with_test_norm, "dsl"),
                "local_scaling": (evaluator.sharded_metrics_with_local_scaling, "csls")}[which]
    plain = fn(m, *_testset(), ARGS, mode)
    on = fn(m, *_testset(), ARGS, mode, **BOOT)
    off = fn(m, *_testset(), ARGS, mode, bootstrap=0)
    raw = evaluator.sharded_metrics(m, *_testset(), ARGS, **BOOT)
    for d in range(2):
        assert off[d] == plain[d]
        assert _without(on[d], "bootstrap", which) == _without(plain[d], which)
        assert _without(on[d][which], "bootstrap", "bootstrap_vs_raw") == plain[d][which]
        _same_summary(on[d]["bootstrap"], raw[d]["bootstrap"])
        _check_direction(on[d], SEED + d, "mid", N)
        _check_direction(on[d][which], SEED + d, "mid", N, raw=on[d])
    if which == "mutual_proximity":                                                   # emp ties by construction: more entries than units
        assert sum(len(on[d][which]["bootstrap"]["entries"]) for d in range(2)) > 2 * N


def _multi_sentence_set():
    """41 videos of 1 to 4 sentences; video 0's only sentence has NaN features: it is not ranked, the video is an empty unit."""
    Vn = 41
    sizes = 1 + (np.arange(Vn) * 3) % 4
    ends = np.cumsum(sizes)
    Ns = int(ends[-1])
    grp = np.searchsorted(ends, np.arange(Ns), side="right")
    t, _, tm, _ = (torch.from_numpy(a) for a in synth.make_samples(92, "test", Ns, Nt, Nv))
    _, v, _, vm = (torch.from_numpy(a) for a in synth.make_samples(93, "test", Vn, Nt, Nv))
    t = t + 0.4 * v[grp].mean(1, keepdim=True)
    assert sizes[0] == 1
    t[0] = float("nan")
    return t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float(), (ends - 1).tolist(), Vn


def test_multi_sentence_sets_resample_videos():
    m = _model()
    t, v, tm, vm, cut, Vn = _multi_sentence_set()
    plain = evaluator.sharded_multi_sentence_metrics(m, t, v, tm, vm, cut, ARGS)
    on = evaluator.sharded_multi_sentence_metrics(m, t, v, tm, vm, cut, ARGS, **BOOT)
    for d in range(2):
        assert _without(on[d], "bootstrap") == plain[d]
    tb = on[0]["bootstrap"]
    assert tb["unit_end"][0] == -1 and len(tb["entries"]) == len(t) - 1                # video 0 has no ranked sentence
    assert tb["unit_end"].tolist() == (np.asarray(cut) - 1).tolist()
    # the text->video dictionary rounds its R@K to float32 (torch's integer division) and takes its mean of r + 1
    _check_direction(on[0], SEED, "low", Vn, point_rel=2.0 ** -23)
    _check_direction(on[1], SEED + 1, "mid", Vn)
    both = evaluator.sharded_metrics_with_mutual_proximity(m, t, v, tm, vm, ARGS, "emp", cut_off_points=cut, **BOOT)
    for d in range(2):
        _same_summary(both[d]["bootstrap"], on[d]["bootstrap"])
    _check_direction(both[0]["mutual_proximity"], SEED, "low", Vn, raw=both[0], point_rel=2.0 ** -23)
    _check_direction(both[1]["mutual_proximity"], SEED + 1, "mid", Vn, raw=both[1])


# ---- the two eval_epoch callers ---------------------------------------------------------------------------------------------------------
class Loader:
    def __init__(self, batches, dataset=None):
        self.batches, self.dataset = batches, dataset

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def test_training_eval_epoch_logs_the_intervals(caplog):
    t, v, tm, vm = (x.cpu() for x in _testset())
    batches = [(t[ix], tm[ix].long(), v[ix], vm[ix].long(), ix.clone(), ix.clone())
               for ix in (torch.arange(lo, min(lo + 32, N)) for lo in range(0, N, 32))]
    dev = torch.device(DEV)

    def run(**over):
        args = SimpleNamespace(world_size=1, rank=0, local_rank=0, logger=logging.getLogger("test_bootstrap"), **over)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="test_bootstrap"):
            out = training.eval_epoch(args, _model(), Loader(batches), dev)
        return out, [r.getMessage() for r in caplog.records]
    base, lines = run()
    assert not any("bootstrap" in line for line in lines) and "bootstrap" not in base[0]
    on, lines = run(bootstrap=NB, bootstrap_seed=SEED)
    want = evaluator.sharded_metrics(_model(), *_testset(), ARGS, **BOOT)
    for d, side in enumerate(("Text-to-Video", "Video-to-Text")):
        assert _without(on[d], "bootstrap") == base[d]
        _same_summary(on[d]["bootstrap"], want[d]["bootstrap"])
        assert RetrievalMetrics.format_bootstrap(on[d]["bootstrap"], prefix=f"{side}: ") in lines
    assert sum("bootstrap" in line for line in lines) == 2
    on, lines = run(bootstrap=NB, bootstrap_seed=SEED, mutual_proximity="emp")
    for d, side in enumerate(("Text-to-Video", "Video-to-Text")):
        mp = on[d]["mutual_proximity"]
        assert RetrievalMetrics.format_bootstrap(on[d]["bootstrap"], prefix=f"{side}: ") in lines
        assert RetrievalMetrics.format_bootstrap(mp["bootstrap"], prefix=f"{side} [MP-emp]: ") in lines
        paired = RetrievalMetrics.format_bootstrap(mp["bootstrap_vs_raw"], prefix=f"{side} [MP-emp] - raw: ")
        assert paired in lines and "frac<=0" in paired
    assert sum("bootstrap" in line for line in lines) == 6


def test_main_retrieval_logs_the_intervals_with_the_flag():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--bootstrap", "200"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()]
    boot = [line for line in lines if "bootstrap" in line]
    assert len(boot) == 2, lines
    assert boot[0].startswith("text->video R@1: ") and boot[1].startswith("video->text R@1: ")
    for line in boot:
        assert "Median R: " in line and "Mean R: " in line and line.endswith("(95% bootstrap, 200 resamples)")
    at = lines.index(boot[0])
    assert lines[at - 1].startswith("text->video R@1 ") and lines[at + 1] == boot[1]      # right after the metrics line
