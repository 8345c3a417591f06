"""GPU: mutual proximity of two-stage retrieval.  nr_cand_mutualprox_rerank alone against the restatement of
tests/rerank_mutualprox_ref.py at the lane / second-slot boundaries of the line (C) and of the stride-64 walk over an item's bank
line (M), with -1 padding, entries past the gallery and below -1, NaN scores, both zeros, both infinities, repeated values, a NaN
inside a bank line, an all-NaN and a constant bank line; the same bits as the exhaustive kernels with every item a candidate; a
line alone against the same line first and last in a workgroup; guard values around every output; then through GalleryIndex and
two_stage_evaluation: the index-time state against the ops composition and the restatement, the corrected scores on the returned
lists, chunk sizes, the inverted file probed whole, the neighbouring index state, a planted hub, single- and multi-sentence
dictionaries with hubness, and two ranks.

Bars.  emp: bit for bit.  gauss: the query's moments within 1e-6 relative of the ordered fp64 sums (the bar of DESIGN.md 6.6 for
moments); corr, given the kernel's own moments, within 4 x the float32 restatement's own distance from the fp64 formulas on the
same inputs (6.6), case by case.  Where a case's own distance is 0 -- lines of one or two slots, whose few finite scores are the
exact values -1/2, -3/4, -1 or are none: C = 1 at n = 5 with every M, C = 1 and C = 2 with M = 1 -- there is nothing to scale, and
the bar is 4 x the largest distance over all the cases' inputs (_gauss_bar_of_the_kernel_cases); the test asserts that this
happens at C <= 2 only.

The index tests use width 256, not 64: nr_prepare_tokens takes multiples of 256.  3 x 2 tokens."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mutualprox_ref as MP
import rerank_mutualprox_ref as MR
import rerank_norm_ref as Q
import rerank_ref as R
from neighborretr_amd import evaluator, hip, modeling, ops, search, synth
from neighborretr_amd.metrics import RetrievalMetrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ARGS = SimpleNamespace(world_size=1)
MODES = search.MUTUAL_PROXIMITY_MODES
F = np.float32

# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------
N_GALLERY = 37
WIDTHS = (1, 2, 63, 64, 65, 128)
BANKS = (1, 63, 64, 65, 200)
# four repeated scores (ties in the query's line and against the bank lines) next to free ones; none but 0 is dyadic: the tails and
# the moments round at every step
VALUES = np.asarray([0.7, 0.3, 0.0, -0.1], dtype=np.float32)
NAN_IN_LINE, ALL_NAN_LINE, CONSTANT_LINE, INF_LINE = 3, 7, 11, 13
OUTSIDE = (N_GALLERY + 5, 2 ** 30, -7)
_CASES, _BANKS, _REFS = {}, {}, {}


def _scores(rng, shape):
    s = np.where(rng.random(shape) < 0.5, VALUES[rng.integers(0, len(VALUES), shape)], rng.uniform(-0.2, 1.0, shape)).astype(F)
    s[(s == 0) & (rng.random(shape) < 0.5)] = -0.0
    return s


def _lines(C, n=5, seed=0):
    """(cand [n, C] int32, fine [n, C] f32): lists in ascending (repeating) gallery index; line 0 ends in -1 padding, line 1 holds
    an entry >= N_GALLERY and scores of +inf and -inf, line 2 is all absent -- by -1, by an entry < -1 and by one far past the
    gallery --, line 3 holds a NaN and a score > 1, line 4 keeps max(1, C // 4) slots.  From C = 4 on line 3 also holds an entry < -1
    between valid ones, from C = 8 on line 0 one far past the gallery: a line of every n = 5 case is compared with the restatement
    around them.  Further lines hold both.  Absent slots score -inf, as nr_local_level_cand writes them.  Built once per (C, n,
    seed)."""
    key = (C, n, seed)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * C + 7 * n + seed)
        cand = np.sort(rng.integers(0, N_GALLERY, (n, C)), axis=1).astype(np.int32)
        fine = _scores(rng, (n, C))
        cand[0, C - min(3, C - 1):] = -1 if C > 1 else cand[0, 0]
        if C >= 8:
            cand[0, 1] = OUTSIDE[1]
        if n > 1:
            fine[1, C - 1] = -np.inf
            fine[1, 0] = np.inf
            cand[1, C // 2] = OUTSIDE[0]
        if n > 2:
            cand[2] = -1
            cand[2, 0] = OUTSIDE[2]
            cand[2, C - 1] = OUTSIDE[1] if C > 1 else cand[2, C - 1]
        if n > 3:
            fine[3, C - 1] = 1.25
            fine[3, C // 3] = np.nan
            if C >= 4:
                cand[3, C // 2] = OUTSIDE[2]
        if n > 4:
            cand[4, max(1, C // 4):] = -1
        for i in range(5, n):
            cand[i, C - 1] = -1
            cand[i, 0] = OUTSIDE[2] if i % 2 else OUTSIDE[1]
        fine[(cand < 0) | (cand >= N_GALLERY)] = -np.inf
        _CASES[key] = (cand, fine)
    return _CASES[key]


def _bank(M):
    """g_line [N_GALLERY, M] f32: the items' bank lines on the scores' scale (so that scores tie with bank entries), a NaN inside
    one line, an all-NaN line, a constant line, a line with both infinities and both zeros."""
    if M not in _BANKS:
        g = _scores(np.random.default_rng(77 + M), (N_GALLERY, M))
        g[NAN_IN_LINE, M // 2] = np.nan
        g[ALL_NAN_LINE] = np.nan
        g[CONSTANT_LINE] = 0.3
        g[INF_LINE, 0] = np.inf
        g[INF_LINE, M - 1] = -np.inf if M > 1 else np.inf
        g[INF_LINE, M // 2] = -0.0 if M > 2 else g[INF_LINE, M // 2]
        _BANKS[M] = g
    return _BANKS[M]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _item_state(g_line):
    """(g_line, g_cnt, g_mean, g_sd) on the device, the moments and counts by the kernels attach_mutualprox uses."""
    line = _dev(g_line, torch.float32)
    return line, ops.mp_line_counts(R=line)[0], *ops.mp_row_moments(line)


def _run(cand, fine, k, mode, g_line, n_gallery=N_GALLERY, want_corr=True, state=None):
    line, cnt, mean, sd = state or _item_state(g_line)
    out = ops.cand_mutualprox_rerank(_dev(fine, torch.float32), _dev(cand, torch.int32), n_gallery, k, mode, g_line=line, g_cnt=cnt,
                                     g_mean=mean, g_sd=sd, want_corr=want_corr)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def _reference(C, M, n):
    """The restatement of one case, computed once and left unchanged: emp's corr and the query moments."""
    key = (C, M, n)
    if key not in _REFS:
        cand, fine = _lines(C, n)
        _REFS[key] = (MR.emp_corr(fine, cand, N_GALLERY, _bank(M)), MR.query_stats(fine, cand, N_GALLERY))
    return _REFS[key]


def _gauss_distance(got, fine, cand, qstat, g_line, n_gallery=N_GALLERY):
    """(the distance of `got` from the fp64 formulas on the moments `qstat`, the float32 restatement's own) -- relative, over the
    finite non-zero entries -- after NaN, infinities and zeros were found in the same places."""
    mean, sd = MP.moments(g_line, 1)
    want = MR.gauss_corr(fine, cand, n_gallery, qstat, mean, sd, np.float64)
    if got is None:
        got32 = None
    else:
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        assert np.array_equal(got[np.isinf(got)], want[np.isinf(want)]) and (got[want == 0] == 0).all()
        got32 = MP.rel_distance(got, want)
    return got32, MP.rel_distance(MR.gauss_corr(fine, cand, n_gallery, qstat, mean, sd), want)


def _gauss_bar_of_the_kernel_cases():
    """4 x the float32 restatement's distance from the fp64 one, the largest over the inputs of every (C, M) case (n = 5, the
    restatement's own moments): the bar of the cases whose own distance is 0.  CPU only, computed once."""
    if "bar" not in _REFS:
        worst = 0.0
        for C in WIDTHS:
            for M in BANKS:
                cand, fine = _lines(C)
                worst = max(worst, _gauss_distance(None, fine, cand, _reference(C, M, 5)[1], _bank(M))[1])
        _REFS["bar"] = 4 * worst
    return _REFS["bar"]


def _check_order(idx, val, corr, cand, k, n_gallery=N_GALLERY):
    """idx / val are the top k of the kernel's own corr under the tie rule; nothing outside the gallery is ever named."""
    want_idx, want_val = MR.rerank(corr, cand, n_gallery, k)
    assert np.array_equal(idx, want_idx) and Q.same_bits(val, want_val), k
    assert not np.isin(idx, OUTSIDE).any()
    absent = (cand < 0) | (cand >= n_gallery)
    assert np.all(np.isneginf(corr[absent]))


@pytest.mark.parametrize("M", BANKS)
@pytest.mark.parametrize("C", WIDTHS)
def test_kernel_equals_the_restatement(C, M):
    g_line = _bank(M)
    pooled = _gauss_bar_of_the_kernel_cases()
    if C == 128:                                                        # every special line is read
        assert all((_lines(C)[0] == item).any() for item in (NAN_IN_LINE, ALL_NAN_LINE, CONSTANT_LINE, INF_LINE))
    for n in (1, 5):                                                    # one live wave; a second workgroup with one live wave
        cand, fine = _lines(C, n)
        want_emp, want_qstat = _reference(C, M, n)
        for k in sorted({1, C}):
            idx, val, corr, qstat = _run(cand, fine, k, "emp", g_line)
            assert Q.same_bits(corr, want_emp) and np.array_equal(qstat[:, 0], want_qstat[:, 0]), (n, k)
            assert MR.moments_close(qstat, want_qstat), (n, k)
            want_idx, want_val = MR.rerank(want_emp, cand, N_GALLERY, k)
            assert np.array_equal(idx, want_idx) and Q.same_bits(val, want_val), (n, k)
            _check_order(idx, val, corr, cand, k)

            idx, val, corr, qstat_g = _run(cand, fine, k, "gauss", g_line)
            assert Q.same_bits(qstat_g, qstat)                           # both modes report the same moments
            dist, own = _gauss_distance(corr, fine, cand, qstat_g, g_line)
            bar = 4 * own if own > 0 else pooled
            print(f"C = {C}, M = {M}, n = {n}: gauss distance from the fp64 formulas {dist:.3e}, the float32 restatement's {own:.3e}, "
                  f"bar {bar:.3e}" + ("" if own > 0 else " (4 x the largest over the cases: this case's own distance is 0)"))
            assert own > 0 or C <= 2, (n, k)                             # only a line of one or two slots has nothing to scale
            assert bar > 0 and dist <= bar, (n, k)
            _check_order(idx, val, corr, cand, k)
            if n == 5:
                assert (cand[:5] == OUTSIDE[2]).any() and (C == 1 or (cand[:5] == OUTSIDE[1]).any())      # below -1, far past the gallery
                assert np.all(idx[2] == -1) and np.all(np.isneginf(val[2])) and qstat[2, 0] == 0 and np.isnan(qstat[2, 1:]).all()
        for mode in MODES:                                              # without the optional output: the same lists
            bare, full = _run(cand, fine, 1, mode, g_line, want_corr=False), _run(cand, fine, 1, mode, g_line)
            assert bare[2] is None and np.array_equal(bare[0], full[0]) and Q.same_bits(bare[1], full[1]) and Q.same_bits(bare[3], full[3])


def test_the_candidate_kernel_and_the_exhaustive_kernels_give_the_same_bits():
    """Every item a candidate (n = 7, N = C = 37, M = 50): emp's corr is ops.mp_emp_apply on the exhaustive counts, gauss's is
    ops.mp_gauss_apply on the query's returned moments and the items' -- as int32 patterns, NaN for NaN."""
    n, C, M = 7, 37, 50
    rng = np.random.default_rng(37)
    S = _scores(rng, (n, C))
    S[0, 3], S[0, 9], S[1, 5], S[2, 7], S[3, 11], S[4, 13], S[5, 0] = 0.0, -0.0, np.inf, -np.inf, np.nan, 1.25, np.nan
    B = _scores(rng, (M, C))                                            # the bank product as the gallery's columns
    B[M // 2, 3], B[:, 17], B[:, 23], B[0, 29], B[1, 29] = np.nan, np.nan, 0.3, np.inf, -np.inf
    cand = np.tile(np.arange(C, dtype=np.int32), (n, 1))
    S_d, B_d = _dev(S, torch.float32), _dev(B, torch.float32)
    g_line = np.ascontiguousarray(B.T)
    row_cnt, col_cnt = ops.mp_line_counts(R=S_d)[0], ops.mp_line_counts(Q=B_d)[1]
    want = ops.mp_emp_apply(S_d, ops.mp_row_counts(S_d, S_d), ops.mp_col_counts(S_d, B_d), row_cnt, col_cnt).cpu().numpy()
    _, _, corr, qstat = _run(cand, S, 1, "emp", g_line, n_gallery=C)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(corr), nan) and np.array_equal(corr.view(np.int32)[~nan], want.view(np.int32)[~nan])
    assert nan[:, 17].all() and nan[3, 11] and nan[5, 0] and (~nan).sum() > n * (C - 3)
    assert np.array_equal(qstat[:, 0], row_cnt.cpu().numpy().astype(F))

    line, cnt, _, _ = _item_state(g_line)
    g_mean, g_sd = ops.mp_moments_combine(ops.mp_col_moments(B_d)[None])             # the lines as the gallery's columns
    _, _, corr, qstat = _run(cand, S, 1, "gauss", g_line, n_gallery=C, state=(line, cnt, g_mean, g_sd))
    want = ops.mp_gauss_apply(S_d, _dev(qstat[:, 1], torch.float32), _dev(qstat[:, 2], torch.float32), g_mean, g_sd).cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(corr), nan) and np.array_equal(corr.view(np.int32)[~nan], want.view(np.int32)[~nan])
    assert nan[:, 17].all() and nan[:, 29].all() and nan[1].all() and nan[2].all() and (~nan).sum() > (n - 2) * (C - 4)
    exhaustive = _np(*ops.mp_row_moments(S_d))
    assert MR.moments_close(qstat[:, 1], exhaustive[0]) and MR.moments_close(qstat[:, 2], exhaustive[1])


@pytest.mark.parametrize("C", WIDTHS)
def test_a_line_does_not_depend_on_its_batch(C):
    """The same line alone, first in a workgroup (row 4 of 8) and last in one (row 7): the same bits."""
    cand, fine = (a.copy() for a in _lines(C, n=8, seed=1))
    cand[4], fine[4] = cand[3], fine[3]
    cand[7], fine[7] = cand[3], fine[3]
    g_line = _bank(65)
    for mode in MODES:
        many = _run(cand, fine, C, mode, g_line)
        one = _run(cand[3:4], fine[3:4], C, mode, g_line)
        for row in (3, 4, 7):
            assert np.array_equal(one[0][0], many[0][row]) and all(Q.same_bits(one[x][0], many[x][row]) for x in (1, 2, 3)), (mode, row)


@pytest.mark.parametrize("mode", MODES)
def test_the_kernel_writes_only_what_it_owns(mode):
    """Every output lies inside a buffer of guard values: out_idx [n, k], out_val [n, k], out_corr [n, C], out_qstat [n, 3] are
    written, nothing before or behind them."""
    n, C, k, M, G = 5, 65, 3, 65, 256
    cand, fine = _lines(C, n)
    line, cnt, mean, sd = _item_state(_bank(M))
    sizes = dict(idx=n * k, val=n * k, corr=n * C, qstat=n * 3)
    guard_i, guard_f = -123456789, -98765.4321
    bufs = {name: torch.full((size + 2 * G,), guard_i if name == "idx" else guard_f, dtype=torch.int32 if name == "idx" else torch.float32,
                             device=DEV) for name, size in sizes.items()}
    inner = {name: bufs[name][G:G + size] for name, size in sizes.items()}
    f_d, c_d = _dev(fine, torch.float32), _dev(cand, torch.int32)
    hip.call("nr_cand_mutualprox_rerank", hip.ptr(f_d), hip.ptr(c_d, torch.int32), n, C, N_GALLERY, ops.MUTUALPROX_MODES[mode],
             hip.ptr(line), hip.ptr(cnt), M, hip.ptr(mean), hip.ptr(sd), k, hip.ptr(inner["idx"]), hip.ptr(inner["val"]),
             hip.ptr(inner["corr"]), hip.ptr(inner["qstat"]), hip.stream_ptr())
    torch.cuda.synchronize()
    for name, size in sizes.items():
        buf = bufs[name].cpu()
        g = guard_i if name == "idx" else torch.tensor(guard_f, dtype=torch.float32).item()
        assert bool((buf[:G] == g).all()) and bool((buf[G + size:] == g).all()), name
    want = _run(cand, fine, k, mode, _bank(M))
    got = (inner["idx"].view(n, k), inner["val"].view(n, k), inner["corr"].view(n, C), inner["qstat"].view(n, 3))
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and all(Q.same_bits(got[x].cpu().numpy(), want[x]) for x in (1, 2, 3))
    assert not bool((got[0] == guard_i).any()) and not bool((got[2] == guard_f).any())          # and all of it was written


def test_a_planted_hub_loses_its_top_1_occurrences_under_gauss():
    """The input tests/test_rerank_mutualprox_cpu.py checks on the restatement: the kernel's top-1 occurrences are the
    restatement's, and the hub's are fewer than raw."""
    cand, fine, g_line, own = MR.planted_hub()
    N = MR.HUB_GALLERY
    raw = MR.top1_occurrences(MR.rerank(fine, cand, N, 1)[0], N)
    want = MR.top1_occurrences(MR.cand_mutualprox_rerank(fine, cand, N, 1, "gauss", g_line)[0], N)
    idx, val, corr, qstat = _run(cand, fine, 1, "gauss", g_line, n_gallery=N)
    got = MR.top1_occurrences(idx, N)
    assert np.array_equal(got, want) and got[MR.HUB] < raw[MR.HUB] == len(own) and np.array_equal(idx[:, 0], own)
    gt = torch.from_numpy(own.astype(np.int32)).to(DEV)

    def hubness(lists):
        occ, good = ops.topk_occurrences(torch.from_numpy(lists).to(DEV), N, gt, gt + 1)
        return RetrievalMetrics.hubness_from_occurrences(occ.cpu().numpy(), good.cpu().numpy(), 1, len(own))
    before, after = hubness(MR.rerank(fine, cand, N, 1)[0]), hubness(idx)
    assert after["max_occurrence"] == 1 and after["good_occurrence_pct"] == 100.0 and after["hub_pct"] == 0.0 < before["hub_pct"]


# ---- 2. through the index -----------------------------------------------------------------------------------------------------------------
# A tiny model of width 256 (nr_prepare_tokens takes multiples of 256), 40 videos x 2 tokens, 40 texts x 3 tokens, a bank of 30
# texts and 30 videos.
D, N, NT, NV, M = 256, 40, 3, 2, 30
SEED, BETA, QB_K, LS_K = 5, 20.0, 2, 3
_SETUP = {}


def _model():
    m = modeling.NeighborRetr(modeling.default_config(), width=D)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(7, d=D).items()}, strict=False)
    return m.to(DEV).eval()


def _samples(seed, stream, n):
    t, v, tm, vm = synth.make_samples(seed, stream, n, NT, NV, d=D)
    return torch.from_numpy(t), torch.from_numpy(v), torch.from_numpy(tm).float(), torch.from_numpy(vm).float()


def _inputs(seed=SEED):
    """(t, v, tm, vm) of the test set and bank = (texts, mask, videos, mask), on the CPU."""
    t, v, tm, vm = _samples(seed, "test", N)
    bt, _, btm, _ = _samples(seed + 100, "train", M)
    _, bv, _, bvm = _samples(seed + 200, "train", M)
    return (t, v, tm, vm), (bt, btm, bv, bvm)


def _setup():
    """Built once: the model, the inputs on the device, both indexes with their bank lines and the GPU's own bank products."""
    if not _SETUP:
        m = _model()
        (t, v, tm, vm), bank = _inputs()
        dev = tuple(x.to(DEV) for x in (t, v, tm, vm))
        bank_dev = tuple(x.to(DEV) for x in bank)
        vi = search.GalleryIndex(m, dev[1], dev[3], "video").attach_mutualprox(bank_dev[0], bank_dev[1])
        ti = search.GalleryIndex(m, dev[0], dev[2], "text").attach_mutualprox(bank_dev[2], bank_dev[3])
        Qt = evaluator._slab_similarity(m, bank_dev[0], dev[1], bank_dev[1], dev[3], 0, M)            # [30, 40]
        Qv = evaluator._slab_similarity(m, dev[0], bank_dev[2], dev[2], bank_dev[3], 0, N)            # [40, 30]
        _SETUP.update(m=m, dev=dev, bank=bank_dev, vi=vi, ti=ti, Qt=Qt, Qv=Qv)
    return SimpleNamespace(**_SETUP)


def _sides(s):
    """(index, queries, their mask)."""
    return ((s.vi, s.dev[0], s.dev[2]), (s.ti, s.dev[1], s.dev[3]))


def _np(*xs):
    return tuple(x.cpu().numpy() for x in xs)


def _bits(x):
    return x.view(torch.int32)


def _mp_state(index):
    return index.mp_line, index.mp_cnt, index.mp_mean, index.mp_sd


def test_index_state_equals_the_ops_composition_and_the_restatement():
    s = _setup()
    want_v = (s.Qt.T.contiguous(), ops.mp_line_counts(Q=s.Qt)[1], *ops.mp_moments_combine(ops.mp_col_moments(s.Qt)[None]))
    want_t = (s.Qv, ops.mp_line_counts(R=s.Qv)[0], *ops.mp_row_moments(s.Qv))
    for index, want, bank_product in ((s.vi, want_v, s.Qt), (s.ti, want_t, s.Qv)):
        line, cnt, mean, sd = _mp_state(index)
        assert line.shape == (N, M) and line.is_contiguous() and line.dtype == mean.dtype == sd.dtype == torch.float32
        assert cnt.shape == mean.shape == sd.shape == (N,) and cnt.dtype == torch.int32 and index.mp_n_bank == M
        assert torch.equal(_bits(line), _bits(want[0])) and torch.equal(cnt, want[1])
        assert torch.equal(_bits(mean), _bits(want[2])) and torch.equal(_bits(sd), _bits(want[3]))
        ref = MR.item_lines(bank_product.cpu().numpy(), index.side)
        assert Q.same_bits(line.cpu().numpy(), ref[0]) and np.array_equal(cnt.cpu().numpy(), ref[1])
        assert MR.moments_close(mean.cpu().numpy(), ref[2]) and MR.moments_close(sd.cpu().numpy(), ref[3])
        assert bool((cnt == M).all()) and bool(torch.isfinite(mean).all()) and bool((sd > 0).all())
        assert index.norm is None and index.active is None and index.ls_mean is None and index.ls_kth is None and index.ivf is None


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [8, N])
def test_search_equals_the_restatement_on_the_returned_lists(mode, C):
    s = _setup()
    for index, q, qm in _sides(s):
        raw = index.candidates(q, qm, C)
        cand, fine, corr, qstat = index.candidates(q, qm, C, mutual_proximity=mode)
        assert torch.equal(cand, raw[0]) and torch.equal(_bits(fine), _bits(raw[1]))       # today's bits
        assert qstat.shape == (N, 3) and corr.shape == (N, C)
        g_line = index.mp_line.cpu().numpy()
        cand_, fine_, corr_, qstat_ = _np(cand, fine, corr, qstat)
        want_qstat = MR.query_stats(fine_, cand_, N)
        assert np.array_equal(qstat_[:, 0], want_qstat[:, 0]) and MR.moments_close(qstat_, want_qstat)
        if mode == "emp":
            assert Q.same_bits(corr_, MR.emp_corr(fine_, cand_, N, g_line))
        else:
            dist, own = _gauss_distance(corr_, fine_, cand_, qstat_, g_line, N)
            print(f"{index.side} gallery, C = {C}: gauss distance from the fp64 formulas {dist:.3e}, the float32 restatement's {own:.3e}")
            assert np.isfinite(corr_).all() and own > 0 and dist <= 4 * own
        k = min(5, C)
        want_idx, want_val = MR.rerank(corr_, cand_, N, k)
        idx, val, cand2, fine2, qstat2 = index.search(q, qm, k, C, return_candidates=True, mutual_proximity=mode)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and Q.same_bits(val.cpu().numpy(), want_val)
        assert torch.equal(cand2, cand) and torch.equal(_bits(fine2), _bits(fine)) and torch.equal(_bits(qstat2), _bits(qstat))
        idx3, val3 = index.search(q, qm, k, C, mutual_proximity=mode)
        assert torch.equal(idx3, idx) and torch.equal(_bits(val3), _bits(val))
        # without the argument: today's return values
        assert len(index.search(q, qm, k, C, return_candidates=True)) == 4 and len(index.candidates(q, qm, C)) == 2
        assert len(index.search(q, qm, k, C)) == 2
    if C == N:
        assert np.array_equal(s.vi.candidates(s.dev[0], s.dev[2], N)[0].cpu().numpy(), np.tile(np.arange(N), (N, 1)))


def test_lists_do_not_depend_on_the_chunk_nor_on_an_inverted_file_probed_whole():
    s = _setup()
    (t, v, tm, vm), bank = s.dev, s.bank
    for index, q, qm in _sides(s):
        for mode in MODES:
            a = index.candidates(q, qm, 8, chunk=256, mutual_proximity=mode)
            b = index.candidates(q, qm, 8, chunk=7, mutual_proximity=mode)
            assert len(a) == 4 and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    again = search.GalleryIndex(s.m, v, vm, "video").attach_mutualprox(bank[0], bank[1])         # built again: the same bits
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(_mp_state(again), _mp_state(s.vi)))
    # the neighbours: nothing of theirs is set by attach_mutualprox, and nothing of its state is touched by them
    assert again.norm is None and again.active is None and again.n_bank == 0 and again.ivf is None
    assert again.ls_mean is None and again.ls_kth is None and again.ls_k is None and again.ls_n_bank == 0
    state = _mp_state(again)
    L = 4
    again.attach_querybank(bank[0], bank[1], BETA, QB_K).attach_localscale(bank[0], bank[1], LS_K).build_ivf(L, iters=2)
    assert all(x is y for x, y in zip(_mp_state(again), state)) and again.mp_n_bank == M
    norm, active, ls_mean, ls_kth, ivf = again.norm, again.active, again.ls_mean, again.ls_kth, again.ivf
    again.attach_mutualprox(bank[0], bank[1])
    assert again.norm is norm and again.active is active and again.ls_mean is ls_mean and again.ls_kth is ls_kth and again.ivf is ivf
    assert (again.norm_beta, again.qb_k, again.n_bank, again.ls_k, again.ls_n_bank) == (BETA, QB_K, M, LS_K, M)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(_mp_state(again), state))
    # every list probed (nprobe = L): the lists without an inverted file; ivf_stats appends its result
    q, qm = s.dev[0], s.dev[2]
    for mode in MODES:
        plain = again.candidates(q, qm, 8, mutual_proximity=mode)
        probed = again.candidates(q, qm, 8, mutual_proximity=mode, nprobe=L, ivf_stats=True)
        assert len(probed) == 5 and probed[4].shape == (N, 3) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(plain, probed))
        a, b = again.search(q, qm, 3, 8, mutual_proximity=mode), again.search(q, qm, 3, 8, mutual_proximity=mode, nprobe=L)
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))
        few = again.search(q, qm, 3, 8, mutual_proximity=mode, nprobe=1, return_candidates=True)
        assert len(few) == 5 and few[0].shape == (N, 3) and few[4].shape == (N, 3)


# ---- 3. the evaluator -------------------------------------------------------------------------------------------------------------------
def _strip(m):
    return {k: v for k, v in m.items() if k not in ("mutual_proximity", "hubness", "mode", "label")}


def _same_hubness(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key


def _want_hubness(cand, score, K, n_gallery, gt_begin, gt_end):
    occ, good = Q.occurrences(MR.rerank(score, cand, n_gallery, K)[0], n_gallery, gt_begin, gt_end)
    return RetrievalMetrics.hubness_from_occurrences(occ, good, K, len(cand))


@pytest.mark.parametrize("mode", MODES)
def test_single_sentence_dictionaries_and_hubness_equal_the_restatement(mode):
    C, K = 8, 3
    s = _setup()
    t, v, tm, vm = s.dev
    got = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, querybank=s.bank, hubness_k=K, mutual_proximity=mode)
    gt = np.arange(N)
    for side, (index, q, qm) in enumerate(_sides(s)):
        cand, fine, corr, _ = _np(*index.candidates(q, qm, C, mutual_proximity=mode))
        assert _strip(got[side]) == R.metrics(R.counts(cand, fine, gt), C)
        n = got[side]["mutual_proximity"]
        assert _strip(n) == R.metrics(R.counts(cand, corr, gt), C)
        assert (n["mode"], n["label"]) == (mode, f"[two-stage C=8 QB-MP-{mode}]") and "k" not in n
        assert "normalised" not in got[side] and "local_scaled" not in got[side]
        _same_hubness(got[side]["hubness"], _want_hubness(cand, fine, K, N, gt, gt + 1))
        _same_hubness(n["hubness"], _want_hubness(cand, corr, K, N, gt, gt + 1))
    for other in (dict(norm="is"), dict(local_scaling="csls", local_scaling_k=LS_K)):
        with pytest.raises(ValueError, match="choose one"):
            evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, querybank=s.bank, mutual_proximity=mode, **other)
    # behind the inverted file probed whole: the IVF figures next to the same corrected ones
    ivf = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, querybank=s.bank, mutual_proximity=mode, n_lists=4, nprobe=4, ivf_iters=2)
    for side in range(2):
        assert ivf[side]["nprobe"] == 4 and ivf[side]["ivf_overlap"] == 1.0
        assert _strip(ivf[side]["mutual_proximity"]) == _strip(got[side]["mutual_proximity"])
    plain = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C)
    assert all(plain[side] == _strip(got[side]) for side in range(2))    # without the argument: the dictionaries as they were


def test_multi_sentence_set_and_hubness_equal_the_restatement():
    C, K = 4, 3
    sizes = [3, 1, 2, 4, 1]                                          # 11 sentences, 5 videos
    ends = np.cumsum(sizes)
    Ns, V = int(ends[-1]), len(sizes)
    s = _setup()
    (t, v, tm, vm), bank = _inputs()
    group = np.searchsorted(ends, np.arange(Ns), side="right")
    first = np.concatenate(([0], ends[:-1]))
    v, vm = v[first], vm[first]
    t = t[first[group]] + 0.5 * (t[:Ns] - t[first[group]])          # sentences of one group: noisy copies of the group's first
    tm = tm[first[group]]
    t, v, tm, vm = (x.to(DEV) for x in (t, v, tm, vm))
    vi = search.GalleryIndex(s.m, v, vm, "video").attach_mutualprox(s.bank[0], s.bank[1])
    ti = search.GalleryIndex(s.m, t, tm, "text").attach_mutualprox(s.bank[2], s.bank[3])
    cand_t, fine_t, corr_t, _ = _np(*vi.candidates(t, tm, C, mutual_proximity="emp"))
    cand_v, fine_v, corr_v, _ = _np(*ti.candidates(v, vm, C, mutual_proximity="emp"))
    got = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, cut_off_points=(ends - 1).tolist(), querybank=s.bank, hubness_k=K,
                                         mutual_proximity="emp")
    raw = R.multi_sentence(cand_t, fine_t, cand_v, fine_v, ends, C)
    fixed = R.multi_sentence(cand_t, corr_t, cand_v, corr_v, ends, C)
    rb, re_, cb, ce = Q.ground_truth(Ns, V, ends)
    for side, (cand, fine, corr, n_gallery, gb, ge) in enumerate(((cand_t, fine_t, corr_t, V, rb, re_), (cand_v, fine_v, corr_v, Ns, cb, ce))):
        assert _strip(got[side]) == raw[side] and _strip(got[side]["mutual_proximity"]) == fixed[side]
        _same_hubness(got[side]["hubness"], _want_hubness(cand, fine, K, n_gallery, gb, ge))
        _same_hubness(got[side]["mutual_proximity"]["hubness"], _want_hubness(cand, corr, K, n_gallery, gb, ge))
    plain = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, cut_off_points=(ends - 1).tolist())
    assert plain[0] == raw[0] and plain[1] == raw[1]                 # without the arguments: the dictionaries as they were


# ---- 4. two gloo ranks on one card ----------------------------------------------------------------------------------------------------
def _evaluate(m, args):
    (t, v, tm, vm), bank = _inputs()
    t, v, tm, vm = (x.to(DEV) for x in (t, v, tm, vm))
    return evaluator.two_stage_evaluation(m, t, v, tm, vm, args, 8, querybank=tuple(x.to(DEV) for x in bank), hubness_k=3,
                                          mutual_proximity="emp")


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    torch.save(_evaluate(_model(), SimpleNamespace(world_size=world, local_rank=rank)), f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def _same_dictionaries(a, b):
    assert _strip(a) == _strip(b) and set(a) == set(b)
    _same_hubness(a["hubness"], b["hubness"])
    if "mutual_proximity" in a:
        _same_dictionaries(a["mutual_proximity"], b["mutual_proximity"])
        assert all(a["mutual_proximity"][key] == b["mutual_proximity"][key] for key in ("mode", "label"))


def test_two_ranks_give_the_single_process_dictionaries(tmp_path):
    import torch.multiprocessing as mp
    want = _evaluate(_setup().m, ARGS)
    world, port = 2, 29747
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        got = torch.load(f"{out}.{r}", weights_only=False)
        for side in range(2):
            assert "mutual_proximity" in got[side] and "hubness" in got[side]["mutual_proximity"]
            _same_dictionaries(got[side], want[side])
