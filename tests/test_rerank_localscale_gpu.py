"""GPU: local scaling of two-stage retrieval.  nr_cand_localscale_rerank alone against the restatement of
tests/rerank_localscale_ref.py (ties everywhere, both zeros, padding, out-of-range entries, an all-absent line, a NaN, fewer
present slots than ls_k, +inf, a score > 1; gallery statistics with a NaN, a value >= 1 and -inf), a planted hub, and one line
against the same line in a batch of 130; then through GalleryIndex and two_stage_evaluation: the index-time statistics against
the exhaustive bank form and the restatement, the corrected scores on the returned lists, chunk sizes, the inverted file with
every list probed, the neighbouring index state, and -- with every item a candidate -- the ranks of the exhaustive bank form of
the sharded evaluator; a multi-sentence set, hubness and two ranks."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import localscale_ref as LS
import rerank_localscale_ref as LR
import rerank_norm_ref as Q
import rerank_ref as R
from neighborretr_amd import evaluator, modeling, ops, search, synth
from neighborretr_amd.metrics import RetrievalMetrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ARGS = SimpleNamespace(world_size=1)
MODES = search.LOCAL_SCALING_MODES

# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------
N_LINES, N_GALLERY = 5, 37
WIDTHS = (1, 2, 63, 64, 65, 128)
# four distinct scores: ties everywhere.  None but 0 is dyadic: 2 x 0.7 - r - c and the sums of the lists round at every step, so a
# contracted or reordered operation changes bits (with dyadic values it would pass unseen)
VALUES = np.asarray([0.7, 0.3, 0.0, -0.1], dtype=np.float32)
NAN_ITEM, BIG_ITEM, NEG_INF_ITEM = 3, 7, 11
_CASES = {}


def _lines(C, n=N_LINES, seed=0):
    """(cand [n, C] int32, fine [n, C] f32): lists in ascending (repeating) gallery index with scores from VALUES and both zeros;
    line 0 ends in -1 padding, line 1 holds an entry >= N_GALLERY and a score of +inf, line 2 is all absent, line 3 holds a NaN and
    a score > 1, line 4 keeps max(1, C // 4) slots (fewer than the middle and the full ls_k); absent slots score -inf, as
    nr_local_level_cand writes them.  Built once per (C, n, seed)."""
    key = (C, n, seed)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * C + 7 * n + seed)
        cand = np.sort(rng.integers(0, N_GALLERY, (n, C)), axis=1).astype(np.int32)
        fine = VALUES[rng.integers(0, len(VALUES), (n, C))]
        fine[(fine == 0) & (rng.random((n, C)) < 0.5)] = -0.0
        cand[0, C - min(3, C - 1):] = -1 if C > 1 else cand[0, 0]
        fine[1, 0] = np.inf
        cand[1, C // 2] = N_GALLERY + 5
        cand[2] = -1
        fine[3, C - 1] = 1.25
        fine[3, C // 3] = np.nan
        cand[4, max(1, C // 4):] = -1
        for i in range(5, n, 9):                                        # longer batches: more of every kind
            cand[i, C - 1] = -1
            cand[i, 0] = -7 if i % 2 else 2 ** 30
        fine[(cand < 0) | (cand >= N_GALLERY)] = -np.inf
        _CASES[key] = (cand, fine)
    return _CASES[key]


def _gstat(seed=3):
    """Gallery statistics on the cosine scale with a NaN, a value >= 1 (the EPS floor) and -inf."""
    g = (0.3 + 0.2 * np.random.default_rng(seed).standard_normal(N_GALLERY)).astype(np.float32)
    g[NAN_ITEM], g[BIG_ITEM], g[NEG_INF_ITEM] = np.nan, 1.5, -np.inf
    return g


def _run(cand, fine, k, g, mode, ls_k, row, n_gallery=N_GALLERY, want_corr=True):
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, t)       # noqa: E731
    out = ops.cand_localscale_rerank(dev(fine, torch.float32), dev(cand, torch.int32), n_gallery, k, dev(g, torch.float32), mode, ls_k,
                                     row, want_corr=want_corr)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def _ks(C):
    return sorted({1, C})


def _ls_ks(C):
    return sorted({1, max(1, C // 2), C})


def _check_against_the_restatement(got, cand, fine, k, g, mode, ls_k, row):
    """qstat bit for bit; corr bit for bit (csls) or within 2e-6 relative of the fp64 formulas on the kernel's own qstat, NaN and
    infinities in the same places (nicdm, ls: the bars of test_localscale_gpu.py); idx / val exactly the top k of the returned corr."""
    idx, val, corr, qstat = got
    assert Q.same_bits(qstat, LR.query_stats(fine, cand, N_GALLERY, ls_k)), (mode, ls_k)
    absent = (cand < 0) | (cand >= N_GALLERY)
    assert np.all(np.isneginf(corr[absent]))
    if mode == "csls":
        assert Q.same_bits(corr, LR.corrected(fine, cand, N_GALLERY, g, mode, qstat, row)), (ls_k, row)
    else:
        want = LR.corrected(fine, cand, N_GALLERY, g, mode, qstat, row, np.float64)
        assert np.array_equal(np.isnan(corr), np.isnan(want)), (mode, ls_k, row)
        assert np.array_equal(np.isinf(corr), np.isinf(want)) and np.array_equal(corr[np.isinf(corr)], want[np.isinf(want)])
        ok = np.isfinite(want)
        np.testing.assert_allclose(corr.astype(np.float64)[ok], want[ok], rtol=2e-6, atol=0)
    want_idx, want_val = LR.rerank(corr, cand, N_GALLERY, k)
    assert np.array_equal(idx, want_idx) and Q.same_bits(val, want_val), (mode, ls_k, row, k)
    assert not np.isin(idx, [N_GALLERY + 5, 2 ** 30, -7]).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", WIDTHS)
def test_kernel_equals_the_restatement(C, mode):
    cand, fine = _lines(C)
    g = _gstat()
    if C == 128:                                                        # every special statistic is read
        assert all((cand == item).any() for item in (NAN_ITEM, BIG_ITEM, NEG_INF_ITEM))
    for ls_k in _ls_ks(C):
        for row in (True, False):
            for k in _ks(C):
                got = _run(cand, fine, k, g, mode, ls_k, row)
                _check_against_the_restatement(got, cand, fine, k, g, mode, ls_k, row)
                idx, val, corr, qstat = got
                assert np.all(idx[2] == -1) and np.all(np.isneginf(val[2])) and np.isnan(qstat[2]).all()       # the all-absent line
                # the tie rule, read off the output itself: values descend, equal values come in ascending position = gallery index
                for i in range(N_LINES):
                    sel = idx[i] >= 0
                    v, j = val[i][sel], idx[i][sel]
                    assert np.all(v[:-1] >= v[1:]) and np.all(j[:-1][v[:-1] == v[1:]] <= j[1:][v[:-1] == v[1:]])
                    assert not sel[np.argmin(sel):].any() if not sel.all() else True        # missing entries come last
            # without the optional output: the same lists
            bare = _run(cand, fine, 1, g, mode, ls_k, row, want_corr=False)
            first = _run(cand, fine, 1, g, mode, ls_k, row)
            assert bare[2] is None and np.array_equal(bare[0], first[0]) and Q.same_bits(bare[1], first[1]) and Q.same_bits(bare[3], first[3])


def test_the_text_side_is_the_row():
    """csls subtracts the row's statistic first, then the column's: the two orientations agree to rounding and differ in bits."""
    cand, fine = _lines(64)
    g = _gstat()
    as_row, as_col = _run(cand, fine, 1, g, "csls", 5, True), _run(cand, fine, 1, g, "csls", 5, False)
    assert Q.same_bits(as_row[3], as_col[3]) and not Q.same_bits(as_row[2], as_col[2])
    ok = np.isfinite(as_row[2])
    assert ok.sum() > 64 and np.array_equal(ok, np.isfinite(as_col[2]))
    np.testing.assert_allclose(as_row[2][ok], as_col[2][ok], rtol=0, atol=1e-6)
    for mode in ("nicdm", "ls"):                                        # a b = b a: no orientation in these
        assert Q.same_bits(_run(cand, fine, 1, g, mode, 5, True)[2], _run(cand, fine, 1, g, mode, 5, False)[2])


def test_a_planted_hub_loses_its_top_1_occurrences_under_csls():
    """Item 5 scores 0.6 against every query, a query's own item 0.55, the rest about 0.1; the hub's bank neighbourhood mean is 0.6,
    the others' 0.1.  Raw, the hub is every query's top-1 (N_1 = 36); csls gives the hub 1.2 - q - 0.6 and the own item 1.1 - q - 0.1:
    every query finds its own item."""
    hub, n, C = 5, N_GALLERY - 1, 8
    rng = np.random.default_rng(11)
    own = np.asarray([i for i in range(N_GALLERY) if i != hub])
    cand = np.zeros((n, C), dtype=np.int32)
    fine = np.zeros((n, C), dtype=np.float32)
    for i, item in enumerate(own):
        others = rng.choice([j for j in range(N_GALLERY) if j not in (hub, item)], C - 2, replace=False)
        cand[i] = np.sort(np.concatenate(([hub, item], others)))
        fine[i] = np.where(cand[i] == hub, 0.6, np.where(cand[i] == item, 0.55, 0.1 + 0.01 * rng.random(C))).astype(np.float32)
    g = np.full(N_GALLERY, 0.1, dtype=np.float32)
    g[hub] = 0.6
    gt = torch.from_numpy(own.astype(np.int32)).to(DEV)

    def hubness(idx):
        occ, good = ops.topk_occurrences(torch.from_numpy(idx).to(DEV), N_GALLERY, gt, gt + 1)
        return RetrievalMetrics.hubness_from_occurrences(occ.cpu().numpy(), good.cpu().numpy(), 1, n)
    raw = hubness(LR.rerank(fine, cand, N_GALLERY, 1)[0])
    assert raw["max_occurrence"] == n and raw["occurrence"][hub] == n and raw["good_occurrence_pct"] == 0.0
    for row in (True, False):
        idx, val, corr, qstat = _run(cand, fine, 1, g, "csls", 3, row)
        assert np.array_equal(idx[:, 0], own)
        fixed = hubness(idx)
        assert fixed["max_occurrence"] == 1 and fixed["occurrence"][hub] == 0 and fixed["good_occurrence_pct"] == 100.0
        assert fixed["hub_pct"] == 0.0 < raw["hub_pct"]


@pytest.mark.parametrize("C", WIDTHS)
def test_a_line_does_not_depend_on_its_batch(C):
    """n = 130: 33 workgroups of four lines, the last one with two."""
    cand, fine = _lines(C, n=130, seed=1)
    g = _gstat()
    ls_k = max(1, C // 2)
    for mode in MODES:
        many = _run(cand, fine, C, g, mode, ls_k, mode != "nicdm")
        if mode == "csls":
            _check_against_the_restatement(many, cand, fine, C, g, mode, ls_k, True)
        for i in (0, 3, 129):
            one = _run(cand[i:i + 1], fine[i:i + 1], C, g, mode, ls_k, mode != "nicdm")
            assert np.array_equal(one[0][0], many[0][i]) and all(Q.same_bits(one[x][0], many[x][i]) for x in (1, 2, 3))


def test_the_candidate_kernel_and_the_exhaustive_kernel_give_one_formulas_bits():
    """Every item a candidate (cand = 0 .. 64 on every line): corr of nr_cand_localscale_rerank is ops.localscale_apply on the same
    scores with the query's returned statistic on its side and g_stat on the gallery's -- as int32 patterns, NaN for NaN.  Five
    queries: two workgroups, the second with one live wave.  Both kernels take the formula from csrc/nr_localscale.h."""
    n, C, ls_k = 5, 65, 10
    rng = np.random.default_rng(65)
    fine = rng.uniform(-0.2, 1.2, (n, C)).astype(np.float32)
    fine[0, 3], fine[0, 9], fine[1, 5], fine[2, 7], fine[3, 11], fine[4, 13] = 0.0, -0.0, 1.0, 1.15, np.nan, np.inf      # 1.15: d floors to 0
    g = rng.uniform(0.2, 1.1, C).astype(np.float32)
    g[17], g[23] = np.float32(1) - np.float32(2.0 ** -22), np.nan                    # above 1 - 2^-20: the EPS floor acts
    assert 1 - g[17] < 2.0 ** -20 and (fine > 1).any() and np.signbit(fine[0, 9])
    cand = np.tile(np.arange(C, dtype=np.int32), (n, 1))
    fine_d, g_d = torch.from_numpy(fine).to(DEV), torch.from_numpy(g).to(DEV)
    for mode in MODES:
        for row in (True, False):
            _, _, corr, qstat = _run(cand, fine, 1, g, mode, ls_k, row, n_gallery=C)
            q_d = torch.from_numpy(np.ascontiguousarray(qstat[:, 1 if mode == "ls" else 0])).to(DEV)
            if row:
                want = ops.localscale_apply(fine_d, mode, q_d, g_d)
            else:
                want = ops.localscale_apply(fine_d.T.contiguous(), mode, g_d, q_d).T
            want = want.contiguous().cpu().numpy()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(corr), nan), (mode, row)
            assert np.array_equal(corr.view(np.int32)[~nan], want.view(np.int32)[~nan]), (mode, row)
            assert nan[:, 23].all() and nan[3, 11] and (~nan).sum() > n * (C - 3)      # the planted NaNs, and little else


# ---- 2. through the index -----------------------------------------------------------------------------------------------------------------
# A tiny model of width 256 (nr_prepare_tokens takes multiples of 256), 37 videos x 12 tokens, 37 texts x 24 tokens, a bank of 9
# texts and 7 videos.  SEED: one for which the fp64 reference separates every rank-deciding pair of corrected scores, in all three
# modes, by more than the two similarity kernels may move it (asserted and printed below).
D, N, NT, NV, M_T, M_V = 256, 37, 24, 12, 9, 7
SEED, LS_K, BETA, QB_K = 5, 3, 20.0, 2
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
    bt, _, btm, _ = _samples(seed + 100, "train", M_T)
    _, bv, _, bvm = _samples(seed + 200, "train", M_V)
    return (t, v, tm, vm), (bt, btm, bv, bvm)


def _setup(seed=SEED):
    """Built once per seed: the model, the inputs on the device, both indexes (query bank first, then the local-scaling
    statistics), the GPU's own bank products and the fp64 similarity (with the token weights the GPU used)."""
    if seed not in _SETUP:
        m = _SETUP[min(_SETUP)].m if _SETUP else _model()
        (t, v, tm, vm), bank = _inputs(seed)
        dev = tuple(x.to(DEV) for x in (t, v, tm, vm))
        bank_dev = tuple(x.to(DEV) for x in bank)
        vi = search.GalleryIndex(m, dev[1], dev[3], "video").attach_querybank(bank_dev[0], bank_dev[1], BETA, QB_K)
        ti = search.GalleryIndex(m, dev[0], dev[2], "text").attach_querybank(bank_dev[2], bank_dev[3], BETA, QB_K)
        vi.attach_localscale(bank_dev[0], bank_dev[1], LS_K)
        ti.attach_localscale(bank_dev[2], bank_dev[3], LS_K)
        Qt = evaluator._slab_similarity(m, bank_dev[0], dev[1], bank_dev[1], dev[3], 0, M_T).cpu().numpy()         # [9, 37]
        Qv = evaluator._slab_similarity(m, dev[0], bank_dev[2], dev[2], bank_dev[3], 0, N).cpu().numpy()           # [37, 7]
        S64 = R.similarity(t, tm, ti.items.w.cpu().view(N, NT), v, vm, vi.items.w.cpu().view(N, NV)).numpy()
        _SETUP[seed] = SimpleNamespace(m=m, dev=dev, bank=bank_dev, vi=vi, ti=ti, Qt=Qt, Qv=Qv, S64=S64)
    return _SETUP[seed]


def _sides(s):
    """(index, queries, their mask)."""
    return ((s.vi, s.dev[0], s.dev[2]), (s.ti, s.dev[1], s.dev[3]))


def _np(*xs):
    return tuple(x.cpu().numpy() for x in xs)


def _bits(x):
    return x.view(torch.int32)


def test_index_statistics_equal_the_exhaustive_bank_form_and_the_restatement():
    s = _setup()
    Qt, Qv = torch.from_numpy(s.Qt).to(DEV), torch.from_numpy(s.Qv).to(DEV)
    S = torch.zeros((N, N), device=DEV)                                 # the bank form reads its shape only
    rows, cols = LS.neighbourhood_stats(np.zeros((N, N), dtype=np.float32), LS_K, s.Qt, s.Qv)
    for which, mode in ((0, "csls"), (0, "nicdm"), (1, "ls")):
        row_stat, col_stat = evaluator._local_scaling_stats(S, N, N, 1, 0, mode, LS_K, bank_slabs=(Qt, Qv), n_bank_texts=M_T)
        got_v, got_t = ((s.vi.ls_mean, s.ti.ls_mean), (s.vi.ls_kth, s.ti.ls_kth))[which]
        assert torch.equal(_bits(got_v), _bits(col_stat)) and torch.equal(_bits(got_t), _bits(row_stat)), mode
        assert Q.same_bits(got_v.cpu().numpy(), cols[which]) and Q.same_bits(got_t.cpu().numpy(), rows[which]), mode
    for index, m_bank in ((s.vi, M_T), (s.ti, M_V)):
        assert index.ls_mean.dtype == index.ls_kth.dtype == torch.float32 and index.ls_mean.shape == index.ls_kth.shape == (N,)
        assert (index.ls_k, index.ls_n_bank) == (LS_K, m_bank) and bool(torch.isfinite(index.ls_mean).all())
        assert not torch.equal(index.ls_kth, index.ls_mean)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [8, N])
def test_corrected_scores_equal_the_restatement_on_the_returned_lists(mode, C):
    s = _setup()
    for index, q, qm in _sides(s):
        row = index.side == "video"
        raw = index.candidates(q, qm, C)
        cand, fine, corr, qstat = index.candidates(q, qm, C, local_scaling=mode)
        assert torch.equal(cand, raw[0]) and torch.equal(_bits(fine), _bits(raw[1]))       # today's bits
        g = (index.ls_kth if mode == "ls" else index.ls_mean).cpu().numpy()
        k = min(5, C)
        cand_, fine_, corr_, qstat_ = _np(cand, fine, corr, qstat)
        assert Q.same_bits(qstat_, LR.query_stats(fine_, cand_, N, LS_K))
        if mode == "csls":
            assert Q.same_bits(corr_, LR.corrected(fine_, cand_, N, g, mode, qstat_, row))
        else:
            want = LR.corrected(fine_, cand_, N, g, mode, qstat_, row, np.float64)
            assert np.isfinite(corr_).all() and np.isfinite(want).all()
            np.testing.assert_allclose(corr_.astype(np.float64), want, rtol=2e-6, atol=0)
        want_idx, want_val = LR.rerank(corr_, cand_, N, k)
        idx, val, cand2, fine2, qstat2 = index.search(q, qm, k, C, return_candidates=True, local_scaling=mode)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and Q.same_bits(val.cpu().numpy(), want_val)
        assert torch.equal(cand2, cand) and torch.equal(_bits(fine2), _bits(fine)) and torch.equal(_bits(qstat2), _bits(qstat))
        idx3, val3 = index.search(q, qm, k, C, local_scaling=mode)
        assert torch.equal(idx3, idx) and torch.equal(_bits(val3), _bits(val))
        # without the argument: today's return values
        assert len(index.search(q, qm, k, C, return_candidates=True)) == 4 and len(index.candidates(q, qm, C)) == 2
        assert len(index.search(q, qm, k, C)) == 2 and len(index.candidates(q, qm, C, norm="is")) == 4


def test_lists_do_not_depend_on_the_chunk_nor_on_an_inverted_file_probed_whole():
    s = _setup()
    (t, v, tm, vm), bank = s.dev, s.bank
    for index, q, qm in _sides(s):
        a = index.candidates(q, qm, 8, chunk=256, local_scaling="nicdm")
        b = index.candidates(q, qm, 8, chunk=7, local_scaling="nicdm")
        assert len(a) == 4 and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    again = search.GalleryIndex(s.m, v, vm, "video").attach_localscale(bank[0], bank[1], LS_K, chunk=7)
    assert torch.equal(_bits(again.ls_mean), _bits(s.vi.ls_mean)) and torch.equal(_bits(again.ls_kth), _bits(s.vi.ls_kth))
    again_t = search.GalleryIndex(s.m, t, tm, "text").attach_localscale(bank[2], bank[3], LS_K, chunk=7)
    assert torch.equal(_bits(again_t.ls_mean), _bits(s.ti.ls_mean)) and torch.equal(_bits(again_t.ls_kth), _bits(s.ti.ls_kth))
    # the other order: local scaling first, then the query bank and the inverted file; nothing disturbs anything
    assert again.norm is None and again.active is None and again.n_bank == 0 and again.ivf is None
    mean, kth = again.ls_mean, again.ls_kth
    again.attach_querybank(bank[0], bank[1], BETA, QB_K).build_ivf(4, iters=2)
    assert again.ls_mean is mean and again.ls_kth is kth and (again.ls_k, again.ls_n_bank) == (LS_K, M_T)
    assert torch.equal(_bits(again.norm), _bits(s.vi.norm)) and torch.equal(again.active, s.vi.active)
    assert (s.vi.norm_beta, s.vi.qb_k, s.vi.n_bank, s.vi.ivf) == (BETA, QB_K, M_T, None)          # _setup attached the bank first
    norm, ivf = again.norm, again.ivf
    again.attach_localscale(bank[0], bank[1], LS_K)
    assert again.norm is norm and again.ivf is ivf and torch.equal(_bits(again.ls_mean), _bits(mean))
    # every list probed: the lists without an index; ivf_stats appends its result
    q, qm = s.dev[0], s.dev[2]
    for mode in MODES:
        plain = again.candidates(q, qm, 8, local_scaling=mode)
        probed = again.candidates(q, qm, 8, local_scaling=mode, nprobe=4, ivf_stats=True)
        assert len(probed) == 5 and probed[4].shape == (N, 3) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(plain, probed))
        a, b = again.search(q, qm, 3, 8, local_scaling=mode), again.search(q, qm, 3, 8, local_scaling=mode, nprobe=4)
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))
        few = again.search(q, qm, 3, 8, local_scaling=mode, nprobe=1, return_candidates=True)
        assert len(few) == 5 and few[0].shape == (N, 3)


# The order of a line does not depend on the query's statistic in exact arithmetic: along a text query's line T is increasing in
#   csls  2 s - c,     nicdm  -d / sqrt(b),     ls  -d^2 / b          (d = 1 - s, b = 1 - c, c = the item's statistic)
# so the exhaustive bank form (query statistic from the bank) and the two-stage lists (from the candidates) rank alike as long as
# no rank-deciding pair -- a query's own item against another -- lies closer than the kernels may move it.  Each similarity kernel
# is held to 2e-6 of fp64 (their tests' bar), the item statistics are the same bits on both paths, and the formulas round
# ROUNDINGS times at a relative 2^-24 each.  Through the partial derivatives, a pair (j, j') may move by
#   csls   2 * 2e-6 per item                    + ROUNDINGS 2^-24 x 4 per item (|2 s|, |r|, |c| <= 4)  (dkey/ds = 2)
#   nicdm  2e-6 / sqrt(b) per item              + ROUNDINGS 2^-24 key per item                      (dkey/ds = 1 / sqrt(b))
#   ls     2e-6 * 2 d / b per item              + ROUNDINGS 2^-24 key per item                      (dkey/ds = 2 d / b)
# and the margin asked for is twice that: both paths may move, in opposite directions.
S_BAR, ROUNDINGS = 2e-6, 8


def _margins(S64, stat, mode):
    """min over the rank-deciding pairs of |key[own] - key[other]| / (2 x what the pair may move), lines = the rows of S64; stat
    [columns]: the items' statistic."""
    s, c = S64, stat.astype(np.float64)[None, :]
    u = 2.0 ** -24
    if mode == "csls":
        key = 2 * s - c
        assert np.abs(s).max() <= 1 and np.abs(c).max() <= 1
        move = 2 * S_BAR + ROUNDINGS * u * 4 + 0 * s
    else:
        d, b = 1 - s, 1 - c
        assert (d > 0).all() and (b > 2.0 ** -20).all()                # no clamp is active: the formulas are smooth here
        key = d / np.sqrt(b) if mode == "nicdm" else d * d / b
        move = S_BAR * (1 / np.sqrt(b) if mode == "nicdm" else 2 * d / b) + ROUNDINGS * u * key
    own_key, own_move = np.diag(key)[:, None], np.diag(move)[:, None]
    ratio = np.abs(key - own_key) / (2 * (move + own_move))
    np.fill_diagonal(ratio, np.inf)
    return float(ratio.min())


def _all_margins(s):
    out = {}
    for mode in MODES:
        which = 1 if mode == "ls" else 0
        v_stat, t_stat = ((s.vi.ls_mean, s.ti.ls_mean), (s.vi.ls_kth, s.ti.ls_kth))[which]
        v_stat, t_stat = v_stat.cpu().numpy(), t_stat.cpu().numpy()
        out[mode] = (_margins(s.S64, v_stat, mode), _margins(s.S64.T, t_stat, mode))
    return out


@pytest.mark.parametrize("mode", MODES)
def test_every_item_a_candidate_gives_the_ranks_of_the_exhaustive_bank_form(mode):
    s = _setup()
    t, v, tm, vm = s.dev
    for name, ratio in zip(("text->video", "video->text"), _all_margins(s)[mode]):
        print(f"seed {SEED}, {mode}, {name}: the fp64 rank-deciding margin is {ratio:.2f} x twice what the kernels may move a pair (needs > 1)")
        assert ratio > 1, (mode, name)
    got = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, N, querybank=s.bank, local_scaling=mode, local_scaling_k=LS_K)
    want = evaluator.sharded_local_scaled_metrics(s.m, t, v, tm, vm, ARGS, mode, LS_K, bank=True, querybank=s.bank)
    for g, w in zip(got, want):
        n = g["local_scaled"]
        assert "normalised" not in g and n["cand_recall"] == 100.0
        assert n["cols"] == w["cols"]
        assert all(n[f"R{K}"] == w[f"R{K}"] for K in (1, 5, 10)) and n["R50"] is None
        assert n["MR"] == w["MR"] and n["MeanR"] == w["MeanR"]
        assert (n["mode"], n["k"], n["label"]) == (mode, LS_K, f"[two-stage C=37 QB-{mode.upper()} k=3]")
        assert g["cols"] != n["cols"]                                                  # the correction does change ranks here
    for index, q, qm in _sides(s):
        assert np.array_equal(index.candidates(q, qm, N)[0].cpu().numpy(), np.tile(np.arange(N), (N, 1)))


def _strip(m):
    return {k: v for k, v in m.items() if k not in ("local_scaled", "hubness", "mode", "k", "label")}


def _same_hubness(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key


def _want_hubness(cand, score, K, n_gallery, gt_begin, gt_end):
    occ, good = Q.occurrences(LR.rerank(score, cand, n_gallery, K)[0], n_gallery, gt_begin, gt_end)
    return RetrievalMetrics.hubness_from_occurrences(occ, good, K, len(cand))


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
    vi = search.GalleryIndex(s.m, v, vm, "video").attach_localscale(s.bank[0], s.bank[1], LS_K)
    ti = search.GalleryIndex(s.m, t, tm, "text").attach_localscale(s.bank[2], s.bank[3], LS_K)
    cand_t, fine_t, corr_t, _ = _np(*vi.candidates(t, tm, C, local_scaling="csls"))
    cand_v, fine_v, corr_v, _ = _np(*ti.candidates(v, vm, C, local_scaling="csls"))
    got = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, cut_off_points=(ends - 1).tolist(), querybank=s.bank, hubness_k=K,
                                         local_scaling="csls", local_scaling_k=LS_K)
    raw = R.multi_sentence(cand_t, fine_t, cand_v, fine_v, ends, C)
    scaled = R.multi_sentence(cand_t, corr_t, cand_v, corr_v, ends, C)
    rb, re_, cb, ce = Q.ground_truth(Ns, V, ends)
    for side, (cand, fine, corr, n_gallery, gb, ge) in enumerate(((cand_t, fine_t, corr_t, V, rb, re_), (cand_v, fine_v, corr_v, Ns, cb, ce))):
        assert _strip(got[side]) == raw[side] and _strip(got[side]["local_scaled"]) == scaled[side]
        _same_hubness(got[side]["hubness"], _want_hubness(cand, fine, K, n_gallery, gb, ge))
        _same_hubness(got[side]["local_scaled"]["hubness"], _want_hubness(cand, corr, K, n_gallery, gb, ge))
    plain = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, cut_off_points=(ends - 1).tolist())
    assert plain[0] == raw[0] and plain[1] == raw[1]                 # without the arguments: the dictionaries as they were


def test_single_sentence_hubness_equals_the_restatement():
    C, K = 8, 3
    s = _setup()
    t, v, tm, vm = s.dev
    got = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, querybank=s.bank, hubness_k=K, local_scaling="ls", local_scaling_k=LS_K)
    gt = np.arange(N)
    for side, (index, q, qm) in enumerate(_sides(s)):
        cand, fine, corr, _ = _np(*index.candidates(q, qm, C, local_scaling="ls"))
        assert _strip(got[side]) == R.metrics(R.counts(cand, fine, gt), C)
        n = got[side]["local_scaled"]
        assert _strip(n) == R.metrics(R.counts(cand, corr, gt), C)
        assert (n["mode"], n["k"], n["label"]) == ("ls", LS_K, "[two-stage C=8 QB-LS k=3]")
        _same_hubness(got[side]["hubness"], _want_hubness(cand, fine, K, N, gt, gt + 1))
        _same_hubness(n["hubness"], _want_hubness(cand, corr, K, N, gt, gt + 1))
    with pytest.raises(ValueError, match="choose one"):
        evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, norm="is", querybank=s.bank, local_scaling="ls", local_scaling_k=LS_K)
    # behind the inverted file: the IVF figures next to the locally scaled ones
    ivf = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, querybank=s.bank, local_scaling="ls", local_scaling_k=LS_K, n_lists=4,
                                         nprobe=4, ivf_iters=2)
    for side in range(2):
        assert ivf[side]["nprobe"] == 4 and ivf[side]["ivf_overlap"] == 1.0
        assert _strip(ivf[side]["local_scaled"]) == _strip(got[side]["local_scaled"])


# ---- 3. two gloo ranks on one card ----------------------------------------------------------------------------------------------------
def _evaluate(m, args):
    (t, v, tm, vm), bank = _inputs()
    t, v, tm, vm = (x.to(DEV) for x in (t, v, tm, vm))
    return evaluator.two_stage_evaluation(m, t, v, tm, vm, args, 8, querybank=tuple(x.to(DEV) for x in bank), hubness_k=3,
                                          local_scaling="nicdm", local_scaling_k=LS_K)


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
    if "local_scaled" in a:
        _same_dictionaries(a["local_scaled"], b["local_scaled"])
        assert all(a["local_scaled"][key] == b["local_scaled"][key] for key in ("mode", "k", "label"))


def test_two_ranks_give_the_single_process_dictionaries(tmp_path):
    import torch.multiprocessing as mp
    want = _evaluate(_setup().m, ARGS)
    world, port = 2, 29743
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        got = torch.load(f"{out}.{r}", weights_only=False)
        for side in range(2):
            assert "local_scaled" in got[side] and "hubness" in got[side]["local_scaled"]
            _same_dictionaries(got[side], want[side])
