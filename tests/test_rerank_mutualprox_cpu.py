"""CPU: mutual proximity of two-stage retrieval without a GPU -- the restatement of tests/rerank_mutualprox_ref.py
against hand-worked lines, the planted-hub input of the GPU test on the restatement, and every refusal before any work:
nr_cand_mutualprox_rerank through ctypes, ops.cand_mutualprox_rerank, GalleryIndex, two_stage_evaluation,
--rerank_mutual_proximity in both eval_epochs and on the command line; the labels and log lines."""
import ctypes
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import rerank_mutualprox_ref as MR
from neighborretr_amd import evaluator, hip, ops, search
from neighborretr_amd.metrics import RetrievalMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
F = np.float32


def f32(*x):
    return np.asarray(x, dtype=np.float32)


# ---- the restatement, by hand -----------------------------------------------------------------------------------------------------------
# gallery of 6, bank of 4.  Item 4's line is all NaN, item 1's holds one NaN, item 3's both infinities and both zeros.
G_LINE = np.stack([f32(0.5, 0.5, 0.5, 0.5), f32(0.25, 0.0, NAN, 0.5), f32(0.1, 0.2, 0.3, 0.4), f32(-INF, INF, 0.0, -0.0),
                   f32(NAN, NAN, NAN, NAN), f32(0.0, -0.0, 1.0, 1.0)])
CAND = np.asarray([[1, 2, 4, 5], [0, 3, 9, -1], [-1, -1, -1, -1]], dtype=np.int32)
FINE = np.stack([f32(0.25, 0.25, 0.5, -0.0), f32(NAN, 0.0, 0.75, 0.75), f32(1, 1, 1, 1)])


def test_emp_on_hand_worked_lines():
    # line 0: the query's line is (0.25, 0.25, 0.5, -0): ties count half -- r2 = 2 x 1 + 2 = 4 of 8 for each 0.25, 7 of 8 for 0.5,
    # 1 of 8 for -0 (it equals itself only)
    assert MR.query_counts(FINE, CAND, 6).tolist() == [[4, 4, 7, 1], [0, 1, 0, 0], [0, 0, 0, 0]]
    # item 1: (0.25, 0, NaN, 0.5), c = 3: 0 below 0.25, one equal: 3 of 6.  item 2: two below: 4 of 8.  item 4: all NaN.
    # item 5: (0, -0, 1, 1) against -0: both zeros equal it: 2 of 8.  item 3 (line 1): -inf below 0, both zeros equal: 4 of 8
    assert MR.item_counts(FINE, CAND, 6, G_LINE).tolist() == [[3, 4, 0, 2], [0, 4, 0, 0], [0, 0, 0, 0]]
    idx, val, corr, qstat = MR.cand_mutualprox_rerank(FINE, CAND, 6, 4, "emp", G_LINE)
    assert corr[0, [0, 1, 3]].tolist() == [0.25, 0.25, 0.03125] and math.isnan(corr[0, 2])         # 0 / 0 of the all-NaN line
    assert idx[0].tolist() == [1, 2, 5, -1] and val[0].tolist() == [0.25, 0.25, 0.03125, -INF]    # ties by lower position
    # line 1: the NaN score stays NaN and is in nobody's line, absent slots are -inf whatever they score; a list of one: 1 of 2
    assert math.isnan(corr[1, 0]) and corr[1, 1:].tolist() == [0.25, -INF, -INF]
    assert idx[1].tolist() == [3, -1, -1, -1] and val[1].tolist() == [0.25, -INF, -INF, -INF]
    # line 2: nothing present
    assert np.all(np.isneginf(corr[2])) and np.all(idx[2] == -1) and np.all(np.isneginf(val[2]))
    # the query's moments, reported in both modes: c, the mean, the population sd; a list of one: sd = 0; c = 0: NaN
    assert qstat[0].tolist() == [4.0, 0.25, float(F(math.sqrt(0.03125)))] and qstat[1].tolist() == [1.0, 0.0, 0.0]
    assert qstat[2, 0] == 0.0 and np.isnan(qstat[2, 1:]).all()
    # fp64: the same counts, one rounding less
    assert MR.emp_corr(FINE, CAND, 6, G_LINE, np.float64)[0, 3] == (1 / 8) * (2 / 8)
    # +inf beats everything, -inf nothing but ties with itself: item 3's line against +-inf
    fine, cand = f32(INF, -INF)[None], np.asarray([[3, 3]], dtype=np.int32)
    assert MR.query_counts(fine, cand, 6).tolist() == [[3, 1]] and MR.item_counts(fine, cand, 6, G_LINE).tolist() == [[7, 1]]
    assert MR.emp_corr(fine, cand, 6, G_LINE)[0].tolist() == [float(F(0.75) * F(7 / 8)), 0.03125]


def test_gauss_on_hand_worked_lines():
    # a list of one: the query's sd is 0, z = 0 / EPS = 0, its tail 1/2.  A constant bank line (item 0: 0.5, sd 0): a score above
    # it has tail 0, the same score 1/2, one below 1: T = -(a + b - a b) = -1/2, -3/4, -1
    for s, want in ((0.75, -0.5), (0.5, -0.75), (0.25, -1.0)):
        _, _, corr, qstat = MR.cand_mutualprox_rerank(f32(s)[None], np.asarray([[0]], dtype=np.int32), 6, 1, "gauss", G_LINE)
        assert corr.tolist() == [[want]] and qstat.tolist() == [[1.0, s, 0.0]]
        assert MR.cand_mutualprox_rerank(f32(s)[None], np.asarray([[0]], dtype=np.int32), 6, 1, "gauss", G_LINE, np.float64)[2].tolist() == [[want]]
    # an all-NaN bank line has NaN moments: NaN, never selected; an infinite score in the query's line makes its mean infinite and
    # its sd NaN: the whole line is NaN
    idx, val, corr, qstat = MR.cand_mutualprox_rerank(FINE, CAND, 6, 4, "gauss", G_LINE)
    assert math.isnan(corr[0, 2]) and np.isfinite(corr[0, [0, 1, 3]]).all() and 4 not in idx[0] and idx[0, 3] == -1
    assert math.isnan(corr[1, 0]) and corr[1, 2:].tolist() == [-INF, -INF] and np.all(np.isneginf(corr[2]))
    assert math.isnan(corr[1, 1]) and np.all(idx[1] == -1)               # item 3's line holds infinities: its sd is NaN
    fine, cand = f32(INF, 0.25)[None], np.asarray([[1, 2]], dtype=np.int32)
    _, _, corr, qstat = MR.cand_mutualprox_rerank(fine, cand, 6, 2, "gauss", G_LINE)
    assert qstat[0, 0] == 2.0 and qstat[0, 1] == INF and math.isnan(qstat[0, 2]) and np.isnan(corr).all()
    # the float32 restatement rounds every operation; the fp64 one agrees to float32 rounding, not to the bit
    rng = np.random.default_rng(0)
    fine, cand = rng.uniform(0, 1, (3, 6)).astype(F), np.tile(np.arange(6, dtype=np.int32), (3, 1))
    lines = rng.uniform(0, 1, (6, 9)).astype(F)
    a = MR.cand_mutualprox_rerank(fine, cand, 6, 6, "gauss", lines)[2]
    b = MR.cand_mutualprox_rerank(fine, cand, 6, 6, "gauss", lines, np.float64)[2]
    assert a.dtype == np.float32 and b.dtype == np.float64 and 0 < np.abs(a - b).max() < 1e-6
    # the moments are sums in position order in fp64: exact for these
    assert MR.query_stats(f32(1.0, 2.0 ** -30, -1.0)[None], np.asarray([[0, 1, 2]]), 3)[0, 1] == F(2.0 ** -30 / 3)


def test_the_planted_hub_loses_top_1_occurrences_on_the_restatement():
    """The input of the GPU test, checked here on the restatement alone: seed and size are chosen so that the reference satisfies
    the condition before any kernel is asked."""
    cand, fine, g_line, own = MR.planted_hub()
    n = len(own)
    assert (n, cand.shape, g_line.shape) == (MR.HUB_GALLERY - 1, (n, MR.HUB_C), (MR.HUB_GALLERY, MR.HUB_M))
    raw = MR.top1_occurrences(MR.rerank(fine, cand, MR.HUB_GALLERY, 1)[0], MR.HUB_GALLERY)
    assert raw[MR.HUB] == n
    for dtype in (np.float32, np.float64):
        idx = MR.cand_mutualprox_rerank(fine, cand, MR.HUB_GALLERY, 1, "gauss", g_line, dtype)[0]
        occ = MR.top1_occurrences(idx, MR.HUB_GALLERY)
        assert occ[MR.HUB] < raw[MR.HUB] and occ[MR.HUB] == 0 and np.array_equal(idx[:, 0], own)


# ---- refusals before any work -----------------------------------------------------------------------------------------------------------
def test_nr_cand_mutualprox_rerank_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(fine=p, cand=p, n=2, C=4, n_gallery=9, mode=0, g_line=p, g_cnt=p, M=3, g_mean=p, g_sd=p, k=2, out_idx=p, out_val=p,
             out_corr=p, out_qstat=p):
        return lib.nr_cand_mutualprox_rerank(fine, cand, n, C, n_gallery, mode, g_line, g_cnt, M, g_mean, g_sd, k, out_idx, out_val,
                                             out_corr, out_qstat, None)
    for mode in (0, 1):
        for name in ("fine", "cand", "out_idx", "out_val"):
            assert call(mode=mode, **{name: None}) == EINVAL, name
        for name in ("n", "n_gallery", "k"):
            assert call(mode=mode, **{name: 0}) == EINVAL and call(mode=mode, **{name: -1}) == EINVAL, name
        assert call(mode=mode, C=0) == EINVAL and call(mode=mode, C=-1) == EINVAL and call(mode=mode, C=129, k=129) == EINVAL
        assert call(mode=mode, k=5) == EINVAL and call(mode=mode, C=128, k=129) == EINVAL        # k > C
        assert call(mode=mode, out_corr=None, out_qstat=None, k=0) == EINVAL                     # optional outputs null: still refused
    for mode in (-1, 2, 7):
        assert call(mode=mode) == EINVAL, mode
    for name in ("g_line", "g_cnt"):
        assert call(mode=0, **{name: None}) == EINVAL, name
    for M in (0, -1, 1 << 23, (1 << 31) - 1):
        assert call(mode=0, M=M) == EINVAL, M
    for name in ("g_mean", "g_sd"):
        assert call(mode=1, **{name: None}) == EINVAL, name
    assert hip.version() == 5 and "nr_cand_mutualprox_rerank" in hip.exported_symbols()
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    assert "int nr_cand_mutualprox_rerank(" in header and "#define NR_ABI_VERSION 5" in header
    assert "#define NR_MUTUALPROX_EMP 0" in header and "#define NR_MUTUALPROX_GAUSS 1" in header
    args, res = hip._SIGNATURES["nr_cand_mutualprox_rerank"]
    assert len(args) == 17 and all(args[i] is ctypes.c_int for i in (2, 3, 4, 5, 8, 11)) and res is ctypes.c_int
    assert len(hip._SIGNATURES["nr_cand_localscale_rerank"][0]) == 15 and len(hip._SIGNATURES["nr_cand_norm_rerank"][0]) == 14
    assert (hip.MUTUALPROX_EMP, hip.MUTUALPROX_GAUSS, hip.MP_LINE_MAX) == (0, 1, 1 << 23)
    # the formulas moved to a header of their own, shared by both kernel files
    shared = open(os.path.join(ROOT, "neighborretr_amd", "csrc", "nr_mutualprox.h")).read()
    for name in ("nr_mp_pair", "nr_mp_emp_score", "nr_mp_tail", "nr_mp_gauss_score", "NR_MP_RSQRT2", "NR_MP_LINE_MAX"):
        assert name in shared, name
    for src in ("nr_mutualprox.hip", "nr_cand_mutualprox.hip"):
        text = open(os.path.join(ROOT, "neighborretr_amd", "csrc", src)).read()
        assert '#include "nr_mutualprox.h"' in text and "float nr_mp_tail(" not in text, src


def test_wrapper_refuses_bad_arguments():
    fine, cand = torch.zeros((3, 4)), torch.zeros((3, 4), dtype=torch.int32)
    line, cnt, vec = torch.zeros((9, 5)), torch.zeros((9,), dtype=torch.int32), torch.zeros((9,))
    emp, gauss = dict(mode="emp", g_line=line, g_cnt=cnt), dict(mode="gauss", g_mean=vec, g_sd=vec)
    for ok in (emp, gauss):
        with pytest.raises(ValueError, match="must both be \\[n, C\\]"):
            ops.cand_mutualprox_rerank(fine, cand[:, :3], 9, 2, **ok)
        with pytest.raises(ValueError, match="k must lie in"):
            ops.cand_mutualprox_rerank(fine, cand, 9, 0, **ok)
        with pytest.raises(ValueError, match="1 <= k <= C"):
            ops.cand_mutualprox_rerank(fine, cand, 9, 5, **ok)
        with pytest.raises(ValueError, match="1 <= k <= C"):
            ops.cand_mutualprox_rerank(torch.zeros((3, 129)), torch.zeros((3, 129), dtype=torch.int32), 9, 2, **ok)
        with pytest.raises(ValueError, match="the gallery is empty"):
            ops.cand_mutualprox_rerank(fine, cand, 0, 2, **ok)
        with pytest.raises(hip.NrHipError):                                            # no CPU path behind the wrapper
            ops.cand_mutualprox_rerank(fine, cand, 9, 2, **ok)
    for mode in ("is", "EMP", "", None, 0, "csls"):
        with pytest.raises(ValueError, match="mode must be one of"):
            ops.cand_mutualprox_rerank(fine, cand, 9, 2, mode, g_line=line, g_cnt=cnt, g_mean=vec, g_sd=vec)
    for bad in (line[:8], line.double(), line[:, :0], line.T[:9], line.to("meta"), None, vec):
        with pytest.raises(ValueError, match="g_line must be a contiguous torch.float32 matrix of 9 rows"):
            ops.cand_mutualprox_rerank(fine, cand, 9, 2, **dict(emp, g_line=bad))
    for bad in (cnt[:8], cnt.long(), vec, cnt.to("meta"), None):
        with pytest.raises(ValueError, match="g_cnt must be a torch.int32 vector of 9"):
            ops.cand_mutualprox_rerank(fine, cand, 9, 2, **dict(emp, g_cnt=bad))
    for name in ("g_mean", "g_sd"):
        for bad in (vec[:8], vec.double(), cnt, vec.to("meta"), None):
            with pytest.raises(ValueError, match=f"{name} must be a torch.float32 vector of 9"):
                ops.cand_mutualprox_rerank(fine, cand, 9, 2, **dict(gauss, **{name: bad}))
    with pytest.raises(ValueError, match="too long for exact counts"):
        ops.cand_mutualprox_rerank(fine.to("meta"), cand.to("meta"), 9, 2, "emp", g_line=torch.zeros((9, 1 << 23), device="meta"),
                                   g_cnt=cnt.to("meta"))         # no memory behind the meta device: only the shape is read


def _bare_index(side="video", attached=True, n=5, d=64, querybank=False, localscale=False):
    """A GalleryIndex with nothing prepared (no GPU here): what the argument checks read, and nothing else."""
    index = object.__new__(search.GalleryIndex)
    index.model, index.side, index.query_side = None, side, "text" if side == "video" else "video"
    index.feat, index.mask = torch.zeros((n, 3, d)), torch.ones((n, 3))
    index.items = NS(n=n, n_tok=3, d=d)
    index.norm = torch.zeros((n,)) if querybank else None
    index.active = torch.zeros((n,), dtype=torch.int32) if querybank else None
    index.norm_beta, index.qb_k, index.n_bank = (20.0, 1, 4) if querybank else (None, None, 0)
    index.ivf = None
    index.ls_mean = torch.zeros((n,)) if localscale else None
    index.ls_kth = torch.zeros((n,)) if localscale else None
    index.ls_k, index.ls_n_bank = (2, 4) if localscale else (None, 0)
    index.mp_line = torch.zeros((n, 4)) if attached else None
    index.mp_cnt = torch.zeros((n,), dtype=torch.int32) if attached else None
    index.mp_mean = torch.zeros((n,)) if attached else None
    index.mp_sd = torch.zeros((n,)) if attached else None
    index.mp_n_bank = 4 if attached else 0
    return index


def test_index_refuses_bad_arguments_before_any_work():
    q, qm = torch.zeros((2, 3, 64)), torch.ones((2, 3))
    assert search.MUTUAL_PROXIMITY_MODES == ("emp", "gauss")
    assert search.check_mutual_proximity(None) is None and search.check_mutual_proximity("gauss") == "gauss"
    assert search.check_correction(None, "ls") == (None, "ls")                          # the older helper keeps its arity
    assert search.check_corrections("is", None, None) == ("is", None, None) and search.check_corrections(None, None, "emp")[2] == "emp"
    for mode in ("is", "qbnorm", "csls", "EMP", "mp", "", 1, True):
        for index in (_bare_index(), _bare_index(attached=False)):
            with pytest.raises(ValueError, match="mutual_proximity must be None or one of"):
                index.candidates(q, qm, 4, mutual_proximity=mode)
            with pytest.raises(ValueError, match="mutual_proximity must be None or one of"):
                index.search(q, qm, 2, 4, mutual_proximity=mode)
    for mode in search.MUTUAL_PROXIMITY_MODES:
        for other in (dict(), dict(querybank=True), dict(localscale=True)):            # the siblings' state is not these lines
            with pytest.raises(ValueError, match="mutual_proximity=.* call attach_mutualprox"):
                _bare_index(attached=False, **other).candidates(q, qm, 4, mutual_proximity=mode)
            with pytest.raises(ValueError, match="mutual_proximity=.* call attach_mutualprox"):
                _bare_index(attached=False, **other).search(q, qm, 2, 4, mutual_proximity=mode)
        for norm in search.NORM_MODES:
            with pytest.raises(ValueError, match="mutual_proximity=.* and norm=.* choose one"):
                _bare_index(querybank=True).candidates(q, qm, 4, norm=norm, mutual_proximity=mode)
            with pytest.raises(ValueError, match="mutual_proximity=.* and norm=.* choose one"):
                _bare_index(querybank=True).search(q, qm, 2, 4, norm=norm, mutual_proximity=mode)
        for ls in search.LOCAL_SCALING_MODES:
            with pytest.raises(ValueError, match="mutual_proximity=.* and local_scaling=.* choose one"):
                _bare_index(localscale=True).candidates(q, qm, 4, local_scaling=ls, mutual_proximity=mode)
            with pytest.raises(ValueError, match="mutual_proximity=.* and local_scaling=.* choose one"):
                _bare_index(localscale=True).search(q, qm, 2, 4, local_scaling=ls, mutual_proximity=mode)
        with pytest.raises(ValueError, match="mutual_proximity acts on candidate lists: the exhaustive path"):
            _bare_index().search(q, qm, 2, 0, mutual_proximity=mode)
        with pytest.raises(ValueError, match="n_candidates must be an integer"):
            _bare_index().candidates(q, qm, 0, mutual_proximity=mode)
        with pytest.raises(ValueError, match="n_candidates must be an integer"):
            _bare_index().candidates(q, qm, 129, mutual_proximity=mode)
        with pytest.raises(ValueError, match="1 <= k <= n_candidates"):
            _bare_index().search(q, qm, 5, 4, mutual_proximity=mode)
        with pytest.raises(ValueError, match="queries are 32 wide"):
            _bare_index().search(q[..., :32], qm, 2, 4, mutual_proximity=mode)
        with pytest.raises(ValueError, match="build_ivf"):
            _bare_index().search(q, qm, 2, 4, mutual_proximity=mode, nprobe=1)
    # attach_mutualprox: shapes, width, device, an empty bank, chunk
    index = _bare_index(attached=False, querybank=True, localscale=True)
    bank, bm = torch.zeros((4, 3, 64)), torch.ones((4, 3))
    for feat, mask, what in ((bank[0], bm, "querybank features must be"), (bank, bm[:3], "querybank mask must be"),
                             (bank, bm[:, :2], "querybank mask must be"), (bank[:0], bm[:0], "the querybank is empty"),
                             (bank[..., :32], bm, "the querybank is 32 wide, the gallery 64"),
                             (bank.to("meta"), bm.to("meta"), "same device"), (None, bm, "querybank features must be")):
        with pytest.raises(ValueError, match=what):
            index.attach_mutualprox(feat, mask)
    for chunk in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="chunk must be an integer"):
            index.attach_mutualprox(bank, bm, chunk=chunk)
    with pytest.raises(ValueError, match="too long for exact counts"):
        index.attach_mutualprox(torch.zeros((1 << 23, 3, 64), device="meta"), torch.ones((1 << 23, 3), device="meta"))
    assert index.mp_line is None and index.mp_cnt is None and index.mp_mean is None and index.mp_sd is None and index.mp_n_bank == 0
    assert index.norm is not None and index.n_bank == 4 and index.ls_mean is not None and index.ls_k == 2      # untouched


def _empty_bank_model():
    z = torch.zeros((0, 3, 64))
    return NS(mb_feat_t=z, mb_mask_t=z[..., 0], mb_feat_v=z, mb_mask_v=z[..., 0])


def _filled_bank_model():
    return NS(mb_feat_t=torch.zeros((2, 3, 64)), mb_mask_t=torch.ones((2, 3)), mb_feat_v=torch.zeros((2, 3, 64)), mb_mask_v=torch.ones((2, 3)))


def test_two_stage_evaluation_refuses_bad_values_before_any_work():
    z = torch.zeros((4, 2, 64))
    head = (None, z, z, z[..., 0], z[..., 0], NS(world_size=1), 8)               # no model: nothing may be touched
    bank = (z, z[..., 0], z, z[..., 0])
    for mode in ("is", "qbnorm", "none", "csls", "EMP", 0.5):
        with pytest.raises(ValueError, match="mutual_proximity must be None or one of"):
            evaluator.two_stage_evaluation(*head, mutual_proximity=mode, querybank=bank)
    for mode in search.MUTUAL_PROXIMITY_MODES:
        for norm in search.NORM_MODES:
            with pytest.raises(ValueError, match="mutual_proximity=.* and norm=.* choose one"):
                evaluator.two_stage_evaluation(*head, norm=norm, mutual_proximity=mode, querybank=bank)
        for ls in search.LOCAL_SCALING_MODES:
            with pytest.raises(ValueError, match="mutual_proximity=.* and local_scaling=.* choose one"):
                evaluator.two_stage_evaluation(*head, local_scaling=ls, local_scaling_k=4, mutual_proximity=mode, querybank=bank)
        with pytest.raises(ValueError, match="n_candidates must be an integer"):
            evaluator.two_stage_evaluation(*head[:6], 0, mutual_proximity=mode, querybank=bank)
        for hubness_k in (9, -1, 129):
            with pytest.raises(ValueError, match="hubness_k must lie in|k must lie in"):
                evaluator.two_stage_evaluation(*head, mutual_proximity=mode, querybank=bank, hubness_k=hubness_k)
        with pytest.raises(ValueError, match="querybank must be"):
            evaluator.two_stage_evaluation(*head, mutual_proximity=mode, querybank=bank[:3])
        with pytest.raises(ValueError, match="memory bank is empty"):
            evaluator.two_stage_evaluation(*head, mutual_proximity=mode, querybank=(z[:0], z[:0, :, 0], z, z[..., 0]))
        with pytest.raises(ValueError, match="memory bank is empty"):              # None: the model's memory bank
            evaluator.two_stage_evaluation(_empty_bank_model(), *head[1:], mutual_proximity=mode)
        with pytest.raises(ValueError, match="nprobe=2 needs an inverted file"):
            evaluator.two_stage_evaluation(*head, mutual_proximity=mode, querybank=bank, nprobe=2)


def test_rerank_mutual_proximity_is_checked_by_both_eval_epochs_and_the_command_line(monkeypatch, capsys):
    from neighborretr_amd import training
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main_retrieval
    model, filled = _empty_bank_model(), _filled_bank_model()
    from_args = evaluator.rerank_mutual_proximity_from_args
    assert from_args(NS(), None) is None
    assert from_args(NS(rerank_mutual_proximity=None, rerank_top=8), None) is None
    assert from_args(NS(rerank_mutual_proximity="none", rerank_norm="qbnorm"), None) is None
    assert from_args(NS(rerank_mutual_proximity="emp", rerank_top=1), filled) == dict(mutual_proximity="emp")
    assert from_args(NS(rerank_mutual_proximity="gauss", rerank_top=8, rerank_norm="none", rerank_local_scaling="none",
                        mutual_proximity="emp", mutual_proximity_bank=1), filled) == dict(mutual_proximity="gauss")      # independent of the exhaustive flags
    for eval_epoch in (lambda a: training.eval_epoch(a, model, None, "cpu"), lambda a: main_retrieval.eval_epoch(a, model, None)):
        for bad in ("is", "qbnorm", "csls", "EMP", "mp", 1):
            with pytest.raises(ValueError, match="rerank_mutual_proximity must be 'emp' or 'gauss'"):
                eval_epoch(NS(rerank_mutual_proximity=bad, rerank_top=16))
        for top in (0, None):
            with pytest.raises(ValueError, match="rerank_mutual_proximity corrects candidate lists: it needs rerank_top >= 1"):
                eval_epoch(NS(rerank_mutual_proximity="emp", rerank_top=top))
        with pytest.raises(ValueError, match="it needs rerank_top >= 1"):
            eval_epoch(NS(rerank_mutual_proximity="gauss"))
        with pytest.raises(ValueError, match="memory bank is empty"):              # every value fine, the bank not filled
            eval_epoch(NS(rerank_mutual_proximity="emp", rerank_top=16))
    # two corrections: each is fine alone (the bank is filled), together they are refused
    for eval_epoch in (lambda a: training.eval_epoch(a, filled, None, "cpu"), lambda a: main_retrieval.eval_epoch(a, filled, None)):
        for norm in ("is", "qbnorm"):
            with pytest.raises(ValueError, match="rerank_mutual_proximity and rerank_norm both correct"):
                eval_epoch(NS(rerank_mutual_proximity="emp", rerank_top=16, rerank_norm=norm))
        for ls in ("csls", "nicdm", "ls"):
            with pytest.raises(ValueError, match="rerank_mutual_proximity and rerank_local_scaling both correct"):
                eval_epoch(NS(rerank_mutual_proximity="gauss", rerank_top=16, rerank_local_scaling=ls))

    def parse(argv):
        monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
        return main_retrieval.get_args()
    got = parse([])
    assert (got.rerank_mutual_proximity, got.rerank_local_scaling, got.rerank_norm) == ("none", "none", "none")
    assert parse(["--rerank_top", "64"]).rerank_mutual_proximity == "none"
    got = parse(["--rerank_top", "1", "--rerank_mutual_proximity", "emp"])
    assert (got.rerank_mutual_proximity, got.rerank_top) == ("emp", 1)
    got = parse(["--rerank_top", "64", "--rerank_mutual_proximity", "gauss", "--mutual_proximity", "emp", "--rerank_lists", "8",
                 "--rerank_probe", "2"])
    assert (got.rerank_mutual_proximity, got.mutual_proximity) == ("gauss", "emp")
    for argv in (["--rerank_mutual_proximity", "emp"], ["--rerank_top", "0", "--rerank_mutual_proximity", "gauss"],
                 ["--rerank_top", "8", "--rerank_mutual_proximity", "mp"], ["--rerank_top", "8", "--rerank_mutual_proximity", "csls"],
                 ["--rerank_top", "64", "--rerank_mutual_proximity", "emp", "--rerank_norm", "is"],
                 ["--rerank_top", "64", "--rerank_mutual_proximity", "gauss", "--rerank_local_scaling", "csls"]):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(argv)
        assert "--rerank_mutual_proximity" in capsys.readouterr().err


def test_labels_and_log_lines():
    assert evaluator.two_stage_mutual_proximity_label(64, "emp") == "[two-stage C=64 QB-MP-emp]"
    assert evaluator.two_stage_mutual_proximity_label(8, "gauss") == "[two-stage C=8 QB-MP-gauss]"
    raw = {"R1": 10.0, "R5": 50.0, "R10": None, "R50": None, "cand_recall": 75.0, "n_candidates": 8, "cols": [0]}
    label = evaluator.two_stage_mutual_proximity_label(8, "emp")
    fixed = dict(raw, R1=20.0, mode="emp", label=label)
    lines = RetrievalMetrics.two_stage_lines(dict(raw, mutual_proximity=fixed), dict(raw, mutual_proximity=dict(fixed, MR=2.0)), "[two-stage C=8]")
    assert lines == ["Text-to-Video [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%",
                     "Video-to-Text [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%",
                     f"Text-to-Video {label}: R@1 20.0 R@5 50.0 - candidate recall 75.0%",
                     f"Video-to-Text {label}: R@1 20.0 R@5 50.0 - candidate recall 75.0% - MedR 2.0"]
    hub = RetrievalMetrics.hubness_from_occurrences([3, 0, 1], [1, 0, 1], 2, 2)
    t2v = dict(raw, hubness=hub, mutual_proximity=dict(fixed, hubness=hub))
    lines = RetrievalMetrics.two_stage_lines(t2v, t2v, "[two-stage C=8]", ("text->video", "video->text"), " ")
    assert len(lines) == 8 and lines[4] == f"text->video {label} R@1 20.0 R@5 50.0 - candidate recall 75.0%"
    assert lines[5].startswith(f"text->video {label} Hubness@2: skew") and lines[7].startswith(f"video->text {label} Hubness@2")
    # without the new key: the lines as before
    assert RetrievalMetrics.two_stage_lines(raw, raw, "[two-stage C=8]") == [
        "Text-to-Video [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%",
        "Video-to-Text [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%"]
