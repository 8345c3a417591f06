"""GPU: query-bank normalisation of two-stage retrieval.  nr_cand_norm_rerank alone against the float32
restatement of tests/rerank_norm_ref.py (ties everywhere, both zeros, padding, out-of-range entries, an all-absent line, a NaN),
without a normaliser against search.rerank, its gate on planted ties, and one line against the same line in a batch of 130; then
through GalleryIndex and two_stage_evaluation: the index-time statistics against fp64, the corrected scores against the
restatement and, with every item a candidate, against the exhaustive QB-Norm of the sharded evaluator; chunk sizes, a
multi-sentence set, hubness and two ranks."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rerank_norm_ref as Q
import rerank_ref as R
from neighborretr_amd import evaluator, modeling, ops, search, synth
from neighborretr_amd.metrics import RetrievalMetrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BETA = 20.0
ARGS = SimpleNamespace(world_size=1)

# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------
N_LINES, N_GALLERY = 5, 37
WIDTHS = (1, 2, 63, 64, 65, 128)
# four distinct scores: ties everywhere; 20 x these is not exact in float32, so a fused multiply-add changes about a third of the
# corrected scores of every case below (with dyadic values it would pass unseen)
VALUES = np.asarray([0.7, 0.3, 0.0, -0.1], dtype=np.float32)
_CASES = {}


def _lines(C, n=N_LINES, seed=0):
    """(cand [n, C] int32, fine [n, C] f32): lists in ascending (repeating) gallery index with scores from VALUES and both zeros;
    line 0 ends in -1 padding, line 1 holds an entry >= N_GALLERY, line 2 is all absent, line 3 holds a NaN; absent slots score
    -inf, as nr_local_level_cand writes them.  Built once per (C, n, seed)."""
    key = (C, n, seed)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * C + 7 * n + seed)
        cand = np.sort(rng.integers(0, N_GALLERY, (n, C)), axis=1).astype(np.int32)
        fine = VALUES[rng.integers(0, len(VALUES), (n, C))]
        fine[(fine == 0) & (rng.random((n, C)) < 0.5)] = -0.0
        cand[0, C - min(3, C - 1):] = -1 if C > 1 else cand[0, 0]
        cand[1, C // 2] = N_GALLERY + 5
        cand[2] = -1
        fine[3, C // 3] = np.nan
        for i in range(5, n, 9):                                        # longer batches: more of every kind
            cand[i, C - 1] = -1
            cand[i, 0] = -7 if i % 2 else 2 ** 30
        fine[(cand < 0) | (cand >= N_GALLERY)] = -np.inf
        _CASES[key] = (cand, fine)
    return _CASES[key]


def _stats(seed=3):
    rng = np.random.default_rng(seed)
    norm = (rng.standard_normal(N_GALLERY) * 3).astype(np.float32)
    active = (rng.random(N_GALLERY) < 0.5).astype(np.int32)
    return norm, active


def _run(cand, fine, k, norm=None, active=None, n_gallery=N_GALLERY):
    dev = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, t)       # noqa: E731
    out = ops.cand_norm_rerank(dev(fine, torch.float32), dev(cand, torch.int32), n_gallery, k, norm=dev(norm, torch.float32),
                               active=dev(active, torch.int32), beta=BETA)
    return tuple(o.cpu().numpy() for o in out)


def _equal(got, want):
    """(idx, val, corr, gate) against the restatement: integers equal, floats bit for bit."""
    assert np.array_equal(got[0], want[0]) and Q.same_bits(got[1], want[1])
    assert Q.same_bits(got[2], want[2]) and np.array_equal(got[3], want[3])


def _ks(C):
    return sorted({1, C})


@pytest.mark.parametrize("C", WIDTHS)
def test_without_a_normaliser_the_kernel_is_rerank(C):
    """search.rerank knows no gallery size: its absent slots are the negative entries.  So it is compared on the lines that hold
    no entry >= N_GALLERY as they are, and on every line with those entries marked absent its way (-1)."""
    cand, fine = _lines(C)
    marked = np.where(cand >= N_GALLERY, -1, cand).astype(np.int32)
    keep = [i for i in range(N_LINES) if (cand[i] < N_GALLERY).all()]
    assert 1 not in keep and len(keep) == N_LINES - 1
    for k in _ks(C):
        idx, val, corr, gate = _run(cand, fine, k)
        for c, rows in ((cand, keep), (marked, list(range(N_LINES)))):
            ri, rv = search.rerank(torch.from_numpy(c).to(DEV), torch.from_numpy(fine).to(DEV), k)
            assert np.array_equal(idx[rows], ri.cpu().numpy()[rows]) and Q.same_bits(val[rows], rv.cpu().numpy()[rows])
        assert not gate.any() and Q.same_bits(corr, fine)
        assert np.all(idx[2] == -1) and np.all(np.isneginf(val[2]))                     # the all-absent line
        _equal((idx, val, corr, gate), Q.cand_norm_rerank(fine, cand, N_GALLERY, k))


@pytest.mark.parametrize("C", WIDTHS)
def test_mode_is_gives_the_bits_of_the_float32_restatement(C):
    cand, fine = _lines(C)
    norm, _ = _stats()
    for k in _ks(C):
        got = _run(cand, fine, k, norm)
        want = Q.cand_norm_rerank(fine, cand, N_GALLERY, k, norm, None, BETA)
        _equal(got, want)
        assert got[3].all()                                                             # every query, the all-absent one included
        absent = (cand < 0) | (cand >= N_GALLERY)
        assert np.all(np.isneginf(got[2][absent])) and not np.isin(got[0], [N_GALLERY + 5, 2 ** 30]).any()
        # the tie rule, read off the output itself: values descend, equal values come in ascending position = gallery index
        for i in range(N_LINES):
            sel = got[0][i] >= 0
            v, j = got[1][i][sel], got[0][i][sel]
            assert np.all(v[:-1] >= v[1:]) and np.all(j[:-1][v[:-1] == v[1:]] <= j[1:][v[:-1] == v[1:]])
            assert not sel[np.argmin(sel):].any() if not sel.all() else True            # missing entries come last


def test_a_large_normaliser_takes_a_hub_off_the_top():
    cand = np.asarray([[3, 8, 20], [3, 8, 20]], dtype=np.int32)
    fine = np.asarray([[0.25, 0.5, 0.25], [0.5, 0.25, -0.0]], dtype=np.float32)        # item 8 wins line 0, item 3 line 1
    norm = np.zeros(N_GALLERY, dtype=np.float32)
    norm[8] = 30.0                                                                      # item 8 is a hub of the bank
    raw = _run(cand, fine, 3)
    assert raw[0].tolist() == [[8, 3, 20], [3, 8, 20]]
    got = _run(cand, fine, 3, norm)
    assert got[0].tolist() == [[3, 20, 8], [3, 20, 8]]
    assert got[1].tolist() == [[5.0, 5.0, -20.0], [10.0, 0.0, -25.0]]
    _equal(got, Q.cand_norm_rerank(fine, cand, N_GALLERY, 3, norm, None, BETA))


def test_a_planted_hub_loses_its_occurrences():
    """Hubness does fall: item 5 scores 0.6 against every query and every bank item, a query's own item 0.55, the rest less.  Raw, the
    hub is every query's top-1 (N_1 = 36); with the bank's normalisers (the hub's is beta * 0.5 above the others') every query finds
    its own item, in mode is and -- the hub being the bank's top-1, hence active -- in mode qbnorm alike."""
    hub, n, C = 5, N_GALLERY - 1, 8
    rng = np.random.default_rng(11)
    own = np.asarray([i for i in range(N_GALLERY) if i != hub])
    cand = np.zeros((n, C), dtype=np.int32)
    fine = np.zeros((n, C), dtype=np.float32)
    for i, g in enumerate(own):
        others = rng.choice([j for j in range(N_GALLERY) if j not in (hub, g)], C - 2, replace=False)
        cand[i] = np.sort(np.concatenate(([hub, g], others)))
        fine[i] = np.where(cand[i] == hub, 0.6, np.where(cand[i] == g, 0.55, 0.1 + 0.01 * rng.random(C))).astype(np.float32)
    bank = np.full((6, N_GALLERY), 0.1, dtype=np.float32)
    bank[:, hub] = 0.6
    norm = Q.lse(bank, BETA, 0).astype(np.float32)
    active = Q.activation(bank, 1, 1).astype(np.int32)
    assert active.tolist() == [int(j == hub) for j in range(N_GALLERY)]
    gt = torch.from_numpy(own.astype(np.int32)).to(DEV)

    def hubness(idx):
        occ, good = ops.topk_occurrences(torch.from_numpy(idx).to(DEV), N_GALLERY, gt, gt + 1)
        return RetrievalMetrics.hubness_from_occurrences(occ.cpu().numpy(), good.cpu().numpy(), 1, n)
    raw = hubness(_run(cand, fine, 1)[0])
    assert raw["max_occurrence"] == n and raw["occurrence"][hub] == n and raw["good_occurrence_pct"] == 0.0 and raw["skewness"] > 5
    for act in (None, active):
        idx, val, corr, gate = _run(cand, fine, 1, norm, act)
        assert gate.all() and np.array_equal(idx[:, 0], own)
        fixed = hubness(idx)
        assert fixed["max_occurrence"] == 1 and fixed["occurrence"][hub] == 0 and fixed["good_occurrence_pct"] == 100.0
        assert fixed["skewness"] < 0 and fixed["hub_pct"] == 0.0 < raw["hub_pct"]      # no right tail is left: no item above 2 mu


@pytest.mark.parametrize("C", WIDTHS)
def test_mode_qbnorm_normalises_the_gated_lines_only(C):
    cand, fine = _lines(C)
    norm, active = _stats()
    for k in _ks(C):
        got = _run(cand, fine, k, norm, active)
        _equal(got, Q.cand_norm_rerank(fine, cand, N_GALLERY, k, norm, active, BETA))
        full, raw = _run(cand, fine, k, norm), _run(cand, fine, k)
        for i in range(N_LINES):
            src = full if got[3][i] else raw                                            # a line is entirely normalised or entirely raw
            assert np.array_equal(got[0][i], src[0][i]) and Q.same_bits(got[1][i], src[1][i]) and Q.same_bits(got[2][i], src[2][i])
        assert got[3][2] == 0                                                           # no top-1: not normalised
    if C > 1:
        assert len(set(_run(cand, fine, 1, norm, active)[3].tolist()) | set(_run(cand, fine, 1, norm, 1 - active)[3].tolist())) == 2


def test_the_gate_follows_the_lower_position_of_a_tied_top_1():
    norm, _ = _stats()
    active = np.zeros(N_GALLERY, dtype=np.int32)
    active[11] = 1
    fine = np.asarray([[0.25, 0.5, -0.5, 0.5], [0.25, 0.5, -0.5, 0.5], [-0.0, -0.5, 0.0, -0.5], [0.0, -0.5, -0.0, -0.5]], dtype=np.float32)
    cand = np.asarray([[2, 11, 12, 30], [2, 9, 10, 11], [11, 12, 13, 14], [5, 6, 11, 14]], dtype=np.int32)
    got = _run(cand, fine, 2, norm, active)
    assert got[3].tolist() == [1, 0, 1, 0]            # active item first; inactive first; the same with -0.0 == +0.0
    _equal(got, Q.cand_norm_rerank(fine, cand, N_GALLERY, 2, norm, active, BETA))


@pytest.mark.parametrize("C", WIDTHS)
def test_a_line_does_not_depend_on_its_batch(C):
    """n = 130: 33 workgroups of four lines, the last one with two."""
    cand, fine = _lines(C, n=130, seed=1)
    norm, active = _stats()
    for k in _ks(C):
        for nrm, act in ((None, None), (norm, None), (norm, active)):
            many = _run(cand, fine, k, nrm, act)
            _equal(many, Q.cand_norm_rerank(fine, cand, N_GALLERY, k, nrm, act, BETA))
            for i in (0, 129):
                one = _run(cand[i:i + 1], fine[i:i + 1], k, nrm, act)
                assert np.array_equal(one[0][0], many[0][i]) and Q.same_bits(one[1][0], many[1][i])
                assert Q.same_bits(one[2][0], many[2][i]) and one[3][0] == many[3][i]


# ---- 2. through the index -----------------------------------------------------------------------------------------------------------------
# A tiny model of width 256 (nr_prepare_tokens takes multiples of 256), 37 videos x 12 tokens, 37 texts x 24 tokens, a bank of 9
# texts and 7 videos.  The seed is one for which the fp64 reference separates every line's top-1 by more than 1e-4 and every
# rank-deciding pair of corrected scores by far more than the two similarity kernels may differ (both asserted below, on the CPU).
D, N, NT, NV, M_T, M_V = 256, 37, 24, 12, 9, 7
SEED, QB_K = 5, 2
_SETUP = {}


def _model():
    m = modeling.NeighborRetr(modeling.default_config(), width=D)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(7, d=D).items()}, strict=False)
    return m.to(DEV).eval()


def _samples(seed, stream, n):
    t, v, tm, vm = synth.make_samples(seed, stream, n, NT, NV, d=D)
    return torch.from_numpy(t), torch.from_numpy(v), torch.from_numpy(tm).float(), torch.from_numpy(vm).float()


def _inputs():
    """(t, v, tm, vm) of the test set and bank = (texts, mask, videos, mask), on the CPU."""
    t, v, tm, vm = _samples(SEED, "test", N)
    bt, _, btm, _ = _samples(SEED + 100, "train", M_T)
    _, bv, _, bvm = _samples(SEED + 200, "train", M_V)
    return (t, v, tm, vm), (bt, btm, bv, bvm)


def _setup():
    """Built once: the model, the inputs on the device, both indexes with their bank attached, the GPU's own bank products and
    the fp64 similarity (with the token weights the GPU used)."""
    if not _SETUP:
        m = _model()
        (t, v, tm, vm), bank = _inputs()
        dev = tuple(x.to(DEV) for x in (t, v, tm, vm))
        bank_dev = tuple(x.to(DEV) for x in bank)
        vi = search.GalleryIndex(m, dev[1], dev[3], "video").attach_querybank(bank_dev[0], bank_dev[1], BETA, QB_K)
        ti = search.GalleryIndex(m, dev[0], dev[2], "text").attach_querybank(bank_dev[2], bank_dev[3], BETA, QB_K)
        Qt = evaluator._slab_similarity(m, bank_dev[0], dev[1], bank_dev[1], dev[3], 0, M_T).cpu().numpy()         # [9, 37]
        Qv = evaluator._slab_similarity(m, dev[0], bank_dev[2], dev[2], bank_dev[3], 0, N).cpu().numpy()           # [37, 7]
        S64 = R.similarity(t, tm, ti.items.w.cpu().view(N, NT), v, vm, vi.items.w.cpu().view(N, NV)).numpy()
        _SETUP.update(m=m, dev=dev, bank=bank_dev, vi=vi, ti=ti, Qt=Qt, Qv=Qv, S64=S64)
    return SimpleNamespace(**_SETUP)


def _sides(s):
    """(index, queries, their mask, the bank product's lines as [gallery, bank])."""
    return ((s.vi, s.dev[0], s.dev[2], s.Qt.T), (s.ti, s.dev[1], s.dev[3], s.Qv))


def _np(*xs):
    return tuple(x.cpu().numpy() for x in xs)


def test_index_statistics_equal_the_definitions():
    s = _setup()
    for index, _, _, lines in _sides(s):
        want = Q.lse(lines, BETA, 1)
        got = index.norm.cpu().numpy()
        assert index.norm.dtype == torch.float32 and index.norm.shape == (N,) and np.isfinite(got).all()
        print(f"{index.side}: max |norm - fp64| = {np.abs(got - want).max():.3e} (bar 1e-6 relative + 1e-6)")
        np.testing.assert_allclose(got.astype(np.float64), want, rtol=1e-6, atol=1e-6)          # the bars of test_hubnorm_gpu
        active = index.active.cpu().numpy()
        assert index.active.dtype == torch.int32 and set(active.tolist()) == {0, 1}
        assert np.array_equal(active != 0, Q.activation(lines, QB_K, 0))
    assert (s.vi.norm_beta, s.vi.qb_k, s.vi.n_bank, s.ti.n_bank) == (BETA, QB_K, M_T, M_V)
    # at one rank: the bits the exhaustive evaluator computes from the same products
    Qt, Qv = torch.from_numpy(s.Qt).to(DEV), torch.from_numpy(s.Qv).to(DEV)
    assert torch.equal(s.vi.norm, evaluator._gathered_lse(ops.hubnorm_col_stats(Qt, BETA), 1))
    assert torch.equal(s.ti.norm, ops.hubnorm_row_lse(Qv, BETA))


@pytest.mark.parametrize("mode", search.NORM_MODES)
@pytest.mark.parametrize("C", [8, N])
def test_corrected_scores_equal_the_restatement_on_the_returned_lists(mode, C):
    s = _setup()
    for index, q, qm, _ in _sides(s):
        raw = index.candidates(q, qm, C)
        cand, fine, corr, gate = index.candidates(q, qm, C, norm=mode)
        assert torch.equal(cand, raw[0]) and torch.equal(fine.view(torch.int32), raw[1].view(torch.int32))
        norm, active = _np(index.norm, index.active)
        k = min(5, C)
        want = Q.cand_norm_rerank(fine.cpu().numpy(), cand.cpu().numpy(), N, k, norm, active if mode == "qbnorm" else None, BETA)
        assert Q.same_bits(corr.cpu().numpy(), want[2]) and np.array_equal(gate.cpu().numpy(), want[3])
        assert gate.all() if mode == "is" else 0 < int(gate.sum()) < N
        idx, val, cand2, fine2, gate2 = index.search(q, qm, k, C, return_candidates=True, norm=mode)
        assert np.array_equal(idx.cpu().numpy(), want[0]) and Q.same_bits(val.cpu().numpy(), want[1])
        assert torch.equal(cand2, cand) and torch.equal(fine2, fine) and torch.equal(gate2, gate)
        idx3, val3 = index.search(q, qm, k, C, norm=mode)
        assert torch.equal(idx3, idx) and torch.equal(val3, val)
        # without the argument: today's return values
        assert len(index.search(q, qm, k, C, return_candidates=True)) == 4 and len(index.candidates(q, qm, C)) == 2


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_every_item_a_candidate_gives_the_exhaustive_qbnorm():
    s = _setup()
    t, v, tm, vm = s.dev
    S64 = s.S64
    # the fp64 reference separates the top-1 of every line (rows: text queries, columns: video queries) by more than 1e-4 ...
    for name, lines in (("rows", S64), ("columns", S64.T)):
        top = np.sort(lines, axis=1)
        gap = top[:, -1] - top[:, -2]
        print(f"fp64 top-1 gap over the {name}: min {gap.min():.3e} (needs > 1e-4)")
        assert np.all(gap > 1e-4), name
    # ... and every rank-deciding pair (a query's own item against another) of its corrected scores by more than twice what the two
    # kernels' scores may differ: each within 2e-6 of fp64, so a pair within 2 * beta * 4e-6 (+ roundings) could change sides
    T64 = BETA * S64 - Q.lse(s.Qt, BETA, 0)[None, :]
    V64 = BETA * S64 - Q.lse(s.Qv, BETA, 1)[:, None]
    for name, lines in (("T rows", T64), ("V columns", V64.T)):
        gaps = np.abs(lines - np.diag(lines)[:, None])
        np.fill_diagonal(gaps, np.inf)
        print(f"fp64 rank-deciding margin of {name}: min {gaps.min():.3e} (needs > {4 * BETA * 4e-6:.1e})")
        assert gaps.min() > 4 * BETA * 4e-6, name
    S = evaluator._slab_similarity(s.m, t, v, tm, vm, 0, N)
    T, V = evaluator.sharded_normalised_slabs(s.m, t, v, tm, vm, ARGS, "qbnorm", BETA, querybank=s.bank, qb_k=QB_K)
    S, T, V = _np(S, T, V)
    worst = 0.0
    for index, q, qm, _ in _sides(s):
        cand, fine, corr, gate = _np(*index.candidates(q, qm, N, norm="qbnorm"))
        assert np.array_equal(cand, np.tile(np.arange(N), (N, 1)))
        full, raw = (T, S) if index.side == "video" else (V.T, S.T)                   # the queries as rows
        want_gate = (full != raw).any(1)                                               # a line is entirely raw or entirely normalised
        assert np.array_equal(full[~want_gate], raw[~want_gate]) and 0 < want_gate.sum() < N
        assert np.array_equal(gate != 0, want_gate)
        bound = np.where(want_gate[:, None], BETA * 4e-6 + 4 * _ulp(BETA * raw), 4e-6)
        err = np.abs(corr.astype(np.float64) - full.astype(np.float64))
        worst = max(worst, float((err / bound).max()))
        print(f"{index.side}: max |corr - exhaustive| = {err.max():.3e}, at most {float((err / bound).max()):.3f} of its bound")
        assert np.all(err <= bound)
    got = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, N, norm="qbnorm", beta=BETA, qb_k=QB_K, querybank=s.bank)
    want = evaluator.sharded_normalised_metrics(s.m, t, v, tm, vm, ARGS, "qbnorm", BETA, querybank=s.bank, qb_k=QB_K)
    for g, w in zip(got, want):
        n = g["normalised"]
        assert n["cols"] == w["cols"] and n["cand_recall"] == 100.0
        assert all(n[f"R{K}"] == w[f"R{K}"] for K in (1, 5, 10)) and n["R50"] is None
        assert n["MR"] == w["MR"] and n["MeanR"] == w["MeanR"]
        assert n["label"] == "[two-stage C=37 QB-Norm b=20 k=2]" and 0 < n["gated"] < 100
        assert g["cols"] != n["cols"]                                                  # the correction does change ranks here


def test_lists_do_not_depend_on_the_chunk():
    s = _setup()
    for index, q, qm, _ in _sides(s):
        a = index.candidates(q, qm, 8, chunk=256, norm="qbnorm")
        b = index.candidates(q, qm, 8, chunk=7, norm="qbnorm")
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    (t, v, tm, vm), bank = s.dev, s.bank
    again = search.GalleryIndex(s.m, v, vm, "video").attach_querybank(bank[0], bank[1], BETA, QB_K, chunk=7)
    assert torch.equal(again.norm.view(torch.int32), s.vi.norm.view(torch.int32)) and torch.equal(again.active, s.vi.active)
    again = search.GalleryIndex(s.m, t, tm, "text").attach_querybank(bank[2], bank[3], BETA, QB_K, chunk=7)
    assert torch.equal(again.norm.view(torch.int32), s.ti.norm.view(torch.int32)) and torch.equal(again.active, s.ti.active)


def _strip(m):
    return {k: v for k, v in m.items() if k not in ("normalised", "hubness", "gated", "label")}


def _same_hubness(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key


def _want_hubness(cand, score, K, n_gallery, gt_begin, gt_end):
    occ, good = Q.occurrences(Q.topk(score, cand, n_gallery, K), n_gallery, gt_begin, gt_end)
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
    vi = search.GalleryIndex(s.m, v, vm, "video").attach_querybank(s.bank[0], s.bank[1], BETA, QB_K)
    ti = search.GalleryIndex(s.m, t, tm, "text").attach_querybank(s.bank[2], s.bank[3], BETA, QB_K)
    cand_t, fine_t, corr_t, gate_t = _np(*vi.candidates(t, tm, C, norm="qbnorm"))
    cand_v, fine_v, corr_v, gate_v = _np(*ti.candidates(v, vm, C, norm="qbnorm"))
    got = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, cut_off_points=(ends - 1).tolist(), norm="qbnorm", beta=BETA,
                                         qb_k=QB_K, querybank=s.bank, hubness_k=K)
    raw = R.multi_sentence(cand_t, fine_t, cand_v, fine_v, ends, C)
    nrm = R.multi_sentence(cand_t, corr_t, cand_v, corr_v, ends, C)
    rb, re_, cb, ce = Q.ground_truth(Ns, V, ends)
    for side, (cand, fine, corr, gate, n_gallery, gb, ge) in enumerate(((cand_t, fine_t, corr_t, gate_t, V, rb, re_),
                                                                        (cand_v, fine_v, corr_v, gate_v, Ns, cb, ce))):
        assert _strip(got[side]) == raw[side] and _strip(got[side]["normalised"]) == nrm[side]
        assert got[side]["normalised"]["gated"] == float(gate.sum()) * 100 / len(gate)
        _same_hubness(got[side]["hubness"], _want_hubness(cand, fine, K, n_gallery, gb, ge))
        _same_hubness(got[side]["normalised"]["hubness"], _want_hubness(cand, corr, K, n_gallery, gb, ge))
    plain = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, cut_off_points=(ends - 1).tolist())
    assert plain[0] == raw[0] and plain[1] == raw[1]                 # without the arguments: the dictionaries as they were


def test_single_sentence_hubness_equals_the_restatement():
    C, K = 8, 3
    s = _setup()
    t, v, tm, vm = s.dev
    got = evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, norm="is", beta=BETA, qb_k=QB_K, querybank=s.bank, hubness_k=K)
    gt = np.arange(N)
    for side, (index, q, qm, _) in enumerate(_sides(s)):
        cand, fine, corr, gate = _np(*index.candidates(q, qm, C, norm="is"))
        assert _strip(got[side]) == R.metrics(R.counts(cand, fine, gt), C)
        n = got[side]["normalised"]
        assert _strip(n) == R.metrics(R.counts(cand, corr, gt), C)
        assert n["gated"] == 100.0 and n["label"] == "[two-stage C=8 IS b=20]"
        _same_hubness(got[side]["hubness"], _want_hubness(cand, fine, K, N, gt, gt + 1))
        _same_hubness(n["hubness"], _want_hubness(cand, corr, K, N, gt, gt + 1))
    with pytest.raises(ValueError, match="hubness_k"):
        evaluator.two_stage_evaluation(s.m, t, v, tm, vm, ARGS, C, norm="is", querybank=s.bank, hubness_k=C + 1)


# ---- 3. two gloo ranks on one card ----------------------------------------------------------------------------------------------------
def _evaluate(m, args):
    (t, v, tm, vm), bank = _inputs()
    t, v, tm, vm = (x.to(DEV) for x in (t, v, tm, vm))
    return evaluator.two_stage_evaluation(m, t, v, tm, vm, args, 8, norm="qbnorm", beta=BETA, qb_k=QB_K,
                                          querybank=tuple(x.to(DEV) for x in bank), hubness_k=3)


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
    if "normalised" in a:
        _same_dictionaries(a["normalised"], b["normalised"])
        assert a["normalised"]["gated"] == b["normalised"]["gated"] and a["normalised"]["label"] == b["normalised"]["label"]


def test_two_ranks_give_the_single_process_dictionaries(tmp_path):
    import torch.multiprocessing as mp
    want = _evaluate(_setup().m, ARGS)
    world, port = 2, 29741
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        got = torch.load(f"{out}.{r}", weights_only=False)
        for side in range(2):
            assert "normalised" in got[side] and "hubness" in got[side]["normalised"]
            _same_dictionaries(got[side], want[side])
