"""CPU: local scaling of two-stage retrieval without a GPU -- the restatement of tests/rerank_localscale_ref.py
against hand-worked lines, and every refusal before any work: nr_cand_localscale_rerank through ctypes,
ops.cand_localscale_rerank, GalleryIndex, two_stage_evaluation, --rerank_local_scaling in both eval_epochs and on the command
line; the labels and log lines."""
import ctypes
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import rerank_localscale_ref as LR
from neighborretr_amd import evaluator, hip, ops, search
from neighborretr_amd.metrics import RetrievalMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
F = np.float32


def f32(*x):
    return np.asarray(x, dtype=np.float32)


# ---- the restatement, by hand -----------------------------------------------------------------------------------------------------------
def test_restatement_on_hand_worked_lines():
    # gallery of 6; line 0: item 4 is the raw top-1 and has the densest bank neighbourhood; line 1: padding, an entry past the
    # gallery, a NaN; line 2: all absent
    cand = np.asarray([[1, 2, 4, 5], [0, 3, 9, -1], [-1, -1, -1, -1]], dtype=np.int32)
    fine = np.stack([f32(0.25, 0.25, 0.5, -0.0), f32(np.nan, 0.0, 0.75, 0.75), f32(1, 1, 1, 1)])
    g = f32(0.0, 0.125, 0.25, 0.5, 0.75, -0.25)
    # the query's list: line 0 (0.5, 0.25 of the lower position): mean 0.375, kth 0.25; line 1 has one selectable slot: c = 1
    qstat = LR.query_stats(fine, cand, 6, 2)
    assert qstat[0].tolist() == [0.375, 0.25] and qstat[1].tolist() == [0.0, 0.0] and np.isnan(qstat[2]).all()
    assert LR.query_stats(fine, cand, 6, 4)[0].tolist() == [0.25, 0.0]                   # (0.5 + 0.25 + 0.25 - 0.0) / 4; kth = -0.0
    assert math.copysign(1.0, LR.query_stats(fine, cand, 6, 4)[0, 1]) == -1.0
    # csls: 2 s - 0.375 - g[cand]: 0.5 - 0.375 - 0.125 = 0; 0.5 - 0.375 - 0.25; 1 - 0.375 - 0.75; -0 - 0.375 + 0.25: the hub drops
    idx, val, corr, qs = LR.cand_localscale_rerank(fine, cand, 6, 4, g, "csls", 2, True)
    assert corr[0].tolist() == [0.0, -0.125, -0.125, -0.125] and idx[0].tolist() == [1, 2, 4, 5]
    assert LR.rerank(fine, cand, 6, 4)[0][0].tolist() == [4, 1, 2, 5]                    # raw: the hub first
    assert val[0].tolist() == [0.0, -0.125, -0.125, -0.125] and LR.same_bits(qs, qstat)
    # line 1: the NaN slot stays NaN and is never selected, absent slots are -inf whatever they score
    assert math.isnan(corr[1, 0]) and corr[1, 1:].tolist() == [-0.5, -INF, -INF]
    assert idx[1].tolist() == [3, -1, -1, -1] and val[1].tolist() == [-0.5, -INF, -INF, -INF]
    # line 2: no neighbourhood, NaN statistics, nothing selected
    assert np.all(np.isneginf(corr[2])) and np.all(idx[2] == -1) and np.all(np.isneginf(val[2]))
    # a NaN gallery statistic: that slot is NaN, never selected
    gn = g.copy()
    gn[1] = np.nan
    idx, val, corr, _ = LR.cand_localscale_rerank(fine, cand, 6, 4, gn, "csls", 2, True)
    assert math.isnan(corr[0, 0]) and idx[0].tolist() == [2, 4, 5, -1]
    # nicdm / ls: s = 0.75, both means 0.75: d = 0.25, a = b = 0.25 -> -(0.25 / sqrt(0.0625)) = -1, -(0.0625 / 0.0625) = -1
    one = (f32(0.75)[None], np.asarray([[0]], dtype=np.int32), 1, 1)
    for mode in ("nicdm", "ls"):
        for row in (True, False):
            assert LR.cand_localscale_rerank(*one, f32(0.75), mode, 1, row)[2].tolist() == [[-1.0]]
    # the EPS floor: a gallery statistic >= 1 gives b = 2^-20: -(0.25 / sqrt(2^-22)) = -512, -(0.0625 / 2^-22) = -2^18
    assert LR.cand_localscale_rerank(*one, f32(1.5), "nicdm", 1, True)[2].tolist() == [[-512.0]]
    assert LR.cand_localscale_rerank(*one, f32(1.5), "ls", 1, False)[2].tolist() == [[-262144.0]]
    # a score > 1: d = max(1 - s, 0) = 0 -> -0.0
    got = LR.cand_localscale_rerank(f32(1.25)[None], one[1], 1, 1, f32(0.5), "nicdm", 1, True)[2][0, 0]
    assert got == 0.0 and math.copysign(1.0, got) == -1.0
    # ls takes the k-th value, csls / nicdm the mean
    two = (f32(0.5, 0.25)[None], np.asarray([[0, 1]], dtype=np.int32), 2, 2)
    assert LR.cand_localscale_rerank(*two, f32(0.0, 0.0), "csls", 2, True)[2].tolist() == [[1.0 - 0.375, 0.5 - 0.375]]
    want = -F(F(0.5) * F(0.5)) / F(F(0.75) * F(1.0))
    assert LR.cand_localscale_rerank(*two, f32(0.0, 0.0), "ls", 2, True)[2][0, 0] == want


def test_restatement_keeps_the_roundings_and_the_order_of_the_sum_apart():
    # the sum runs in list order from the first: 1 + 2^-24 + 2^-24 = 1 in float32 (each addend is lost), 2^-24 + 2^-24 + 1 is not
    tiny = F(2.0 ** -24)
    fine, cand = f32(tiny, 1.0, tiny)[None], np.asarray([[0, 1, 2]], dtype=np.int32)
    qstat = LR.query_stats(fine, cand, 3, 3)
    assert qstat[0, 0] == F(1.0) / F(3.0) != F(F(F(tiny + tiny) + F(1.0)) / F(3.0)) and qstat[0, 1] == tiny
    # csls: which statistic is subtracted first matters: the text side is the row
    s, q, g = F(0.3), F(0.7), F(1e-8)
    fine, cand = f32(q, s)[None], np.asarray([[0, 1]], dtype=np.int32)
    gs = f32(g, g)
    as_row = LR.cand_localscale_rerank(fine, cand, 2, 2, gs, "csls", 1, True)
    as_col = LR.cand_localscale_rerank(fine, cand, 2, 2, gs, "csls", 1, False)
    assert as_row[3][0].tolist() == [q, q]
    assert as_row[2][0, 1] == F(F(F(2) * s - q) - g) and as_col[2][0, 1] == F(F(F(2) * s - g) - q)
    assert as_row[2][0, 1] != as_col[2][0, 1]
    # the fp64 variant: the same formula, one rounding less
    assert LR.cand_localscale_rerank(fine, cand, 2, 2, gs, "csls", 1, True, np.float64)[2][0, 1] == 2 * float(s) - float(q) - float(g)
    # ties by lower position, -0.0 == +0.0, in the query's list as in the output
    fine, cand = f32(-0.0, 0.0, 0.0)[None], np.asarray([[3, 4, 5]], dtype=np.int32)
    idx, val = LR.query_list(fine[0], cand[0], 6, 2)
    assert idx.tolist() == [3, 4] and math.copysign(1.0, val[0]) == -1.0
    assert LR.rerank(fine, cand, 6, 3)[0].tolist() == [[3, 4, 5]]


# ---- refusals before any work -----------------------------------------------------------------------------------------------------------
def test_nr_cand_localscale_rerank_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(fine=p, cand=p, n=2, C=4, n_gallery=9, g_stat=p, mode=0, ls_k=2, query_is_row=1, k=2, out_idx=p, out_val=p, out_corr=p,
             out_qstat=p):
        return lib.nr_cand_localscale_rerank(fine, cand, n, C, n_gallery, g_stat, mode, ls_k, query_is_row, k, out_idx, out_val,
                                             out_corr, out_qstat, None)
    for name in ("fine", "cand", "g_stat", "out_idx", "out_val"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("n", "n_gallery", "k"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
    assert call(C=0) == EINVAL and call(C=-1) == EINVAL and call(C=129) == EINVAL and call(C=129, k=129, ls_k=129) == EINVAL
    assert call(k=5) == EINVAL and call(C=128, k=129) == EINVAL                        # k > C
    for ls_k in (0, -1, 5, 129):
        assert call(ls_k=ls_k) == EINVAL, ls_k                                         # ls_k outside [1, C]
    for mode in (-1, 3, 7):
        assert call(mode=mode) == EINVAL, mode
    for row in (-1, 2):
        assert call(query_is_row=row) == EINVAL, row
    # optional outputs null with a bad argument: still refused, nothing launched
    assert call(out_corr=None, out_qstat=None, k=0) == EINVAL
    assert hip.version() == 5 and "nr_cand_localscale_rerank" in hip.exported_symbols()
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    assert "int nr_cand_localscale_rerank(" in header and "#define NR_ABI_VERSION 5" in header
    args, res = hip._SIGNATURES["nr_cand_localscale_rerank"]
    assert len(args) == 15 and all(a is ctypes.c_int for a in args[6:10]) and res is ctypes.c_int
    assert len(hip._SIGNATURES["nr_cand_norm_rerank"][0]) == 14                        # the sibling stays as it was
    assert (hip.LOCALSCALE_CSLS, hip.LOCALSCALE_NICDM, hip.LOCALSCALE_LS) == (0, 1, 2)


def test_wrapper_refuses_bad_arguments():
    fine, cand, g = torch.zeros((3, 4)), torch.zeros((3, 4), dtype=torch.int32), torch.zeros((9,))
    ok = dict(g_stat=g, mode="csls", ls_k=2, query_is_row=True)
    with pytest.raises(ValueError, match="must both be \\[n, C\\]"):
        ops.cand_localscale_rerank(fine, cand[:, :3], 9, 2, **ok)
    with pytest.raises(ValueError, match="k must lie in"):
        ops.cand_localscale_rerank(fine, cand, 9, 0, **ok)
    with pytest.raises(ValueError, match="1 <= k <= C"):
        ops.cand_localscale_rerank(fine, cand, 9, 5, **ok)
    with pytest.raises(ValueError, match="1 <= k <= C"):
        ops.cand_localscale_rerank(torch.zeros((3, 129)), torch.zeros((3, 129), dtype=torch.int32), 9, 2, **ok)
    with pytest.raises(ValueError, match="the gallery is empty"):
        ops.cand_localscale_rerank(fine, cand, 0, 2, **ok)
    for mode in ("is", "CSLS", "", None, 0):
        with pytest.raises(ValueError, match="mode must be one of"):
            ops.cand_localscale_rerank(fine, cand, 9, 2, **dict(ok, mode=mode))
    for ls_k in (0, 5, -1, 2.0, True):
        with pytest.raises(ValueError, match="ls_k must be an integer in \\[1, C = 4\\]"):
            ops.cand_localscale_rerank(fine, cand, 9, 2, **dict(ok, ls_k=ls_k))
    for row in (2, -1, None, "yes"):
        with pytest.raises(ValueError, match="query_is_row must be True or False"):
            ops.cand_localscale_rerank(fine, cand, 9, 2, **dict(ok, query_is_row=row))
    for bad in (g[:8], g.double(), None):
        with pytest.raises(ValueError, match="g_stat must be a torch.float32 vector of 9"):
            ops.cand_localscale_rerank(fine, cand, 9, 2, **dict(ok, g_stat=bad))
    with pytest.raises(hip.NrHipError):                                                # no CPU path behind the wrapper
        ops.cand_localscale_rerank(fine, cand, 9, 2, **ok)


def _bare_index(side="video", attached=True, n=5, d=64, ls_k=2, querybank=False):
    """A GalleryIndex with nothing prepared (no GPU here): what the argument checks read, and nothing else."""
    index = object.__new__(search.GalleryIndex)
    index.model, index.side, index.query_side = None, side, "text" if side == "video" else "video"
    index.feat, index.mask = torch.zeros((n, 3, d)), torch.ones((n, 3))
    index.items = NS(n=n, n_tok=3, d=d)
    index.norm = torch.zeros((n,)) if querybank else None
    index.active = torch.zeros((n,), dtype=torch.int32) if querybank else None
    index.norm_beta, index.qb_k, index.n_bank = (20.0, 1, 4) if querybank else (None, None, 0)
    index.ivf = None
    index.ls_mean = torch.zeros((n,)) if attached else None
    index.ls_kth = torch.zeros((n,)) if attached else None
    index.ls_k, index.ls_n_bank = (ls_k, 4) if attached else (None, 0)
    return index


def test_index_refuses_bad_arguments_before_any_work():
    q, qm = torch.zeros((2, 3, 64)), torch.ones((2, 3))
    assert search.LOCAL_SCALING_MODES == ("csls", "nicdm", "ls") and search.NORM_MODES == ("is", "qbnorm")
    assert search.check_local_scaling(None) is None and search.check_local_scaling("ls") == "ls"
    for mode in ("is", "qbnorm", "CSLS", "mp", "", 1, True):
        for index in (_bare_index(), _bare_index(attached=False)):
            with pytest.raises(ValueError, match="local_scaling must be None or one of"):
                index.candidates(q, qm, 4, local_scaling=mode)
            with pytest.raises(ValueError, match="local_scaling must be None or one of"):
                index.search(q, qm, 2, 4, local_scaling=mode)
    for mode in search.LOCAL_SCALING_MODES:
        with pytest.raises(ValueError, match="attach_localscale"):
            _bare_index(attached=False).candidates(q, qm, 4, local_scaling=mode)
        with pytest.raises(ValueError, match="attach_localscale"):
            _bare_index(attached=False).search(q, qm, 2, 4, local_scaling=mode)
        with pytest.raises(ValueError, match="attach_localscale"):                     # a query bank of 6.15 is not these statistics
            _bare_index(attached=False, querybank=True).search(q, qm, 2, 4, local_scaling=mode)
        for norm in search.NORM_MODES:
            with pytest.raises(ValueError, match="choose one"):
                _bare_index(querybank=True).candidates(q, qm, 4, norm=norm, local_scaling=mode)
            with pytest.raises(ValueError, match="choose one"):
                _bare_index(querybank=True).search(q, qm, 2, 4, norm=norm, local_scaling=mode)
        with pytest.raises(ValueError, match="exhaustive path"):
            _bare_index().search(q, qm, 2, 0, local_scaling=mode)
        with pytest.raises(ValueError, match="n_candidates >= 3 expected, got 2"):
            _bare_index(ls_k=3).search(q, qm, 2, 2, local_scaling=mode)
        with pytest.raises(ValueError, match="n_candidates >= 3 expected, got 2"):
            _bare_index(ls_k=3).candidates(q, qm, 2, local_scaling=mode)
        with pytest.raises(ValueError, match="n_candidates must be an integer"):
            _bare_index().candidates(q, qm, 129, local_scaling=mode)
        with pytest.raises(ValueError, match="1 <= k <= n_candidates"):
            _bare_index().search(q, qm, 5, 4, local_scaling=mode)
        with pytest.raises(ValueError, match="queries are 32 wide"):
            _bare_index().search(q[..., :32], qm, 2, 4, local_scaling=mode)
        with pytest.raises(ValueError, match="build_ivf"):
            _bare_index().search(q, qm, 2, 4, local_scaling=mode, nprobe=1)
    # attach_localscale: shapes, width, device, an empty bank, k, chunk
    index = _bare_index(attached=False, querybank=True)
    bank, bm = torch.zeros((4, 3, 64)), torch.ones((4, 3))
    for feat, mask, what in ((bank[0], bm, "querybank features must be"), (bank, bm[:3], "querybank mask must be"),
                             (bank, bm[:, :2], "querybank mask must be"), (bank[:0], bm[:0], "the querybank is empty"),
                             (bank[..., :32], bm, "the querybank is 32 wide, the gallery 64"),
                             (bank.to("meta"), bm.to("meta"), "same device"), (None, bm, "querybank features must be")):
        with pytest.raises(ValueError, match=what):
            index.attach_localscale(feat, mask)
    for kw, what in ((dict(k=0), "k must be an integer in"), (dict(k=129), "k must be an integer in"), (dict(k=2.5), "k must be an integer in"),
                     (dict(k=True), "k must be an integer in"), (dict(chunk=0), "chunk must be an integer")):
        with pytest.raises(ValueError, match=what):
            index.attach_localscale(bank, bm, **kw)
    assert index.ls_mean is None and index.ls_kth is None and index.ls_k is None and index.ls_n_bank == 0
    assert index.norm is not None and index.n_bank == 4                                # the other state was not touched


def _empty_bank_model():
    z = torch.zeros((0, 3, 64))
    return NS(mb_feat_t=z, mb_mask_t=z[..., 0], mb_feat_v=z, mb_mask_v=z[..., 0])


def _filled_bank_model():
    return NS(mb_feat_t=torch.zeros((2, 3, 64)), mb_mask_t=torch.ones((2, 3)), mb_feat_v=torch.zeros((2, 3, 64)), mb_mask_v=torch.ones((2, 3)))


def test_two_stage_evaluation_refuses_bad_values_before_any_work():
    z = torch.zeros((4, 2, 64))
    head = (None, z, z, z[..., 0], z[..., 0], NS(world_size=1), 8)               # no model: nothing may be touched
    bank = (z, z[..., 0], z, z[..., 0])
    for mode in ("is", "qbnorm", "none", "CSLS", 0.5):
        with pytest.raises(ValueError, match="local_scaling must be None or one of"):
            evaluator.two_stage_evaluation(*head, local_scaling=mode, querybank=bank)
    for mode in search.LOCAL_SCALING_MODES:
        for norm in search.NORM_MODES:
            with pytest.raises(ValueError, match="choose one"):
                evaluator.two_stage_evaluation(*head, norm=norm, local_scaling=mode, querybank=bank)
        for k in (0, 129, -1, 2.0, True):
            with pytest.raises(ValueError, match="k must be an integer in"):
                evaluator.two_stage_evaluation(*head, local_scaling=mode, local_scaling_k=k, querybank=bank)
        with pytest.raises(ValueError, match="local_scaling_k must lie in \\[1, n_candidates = 8\\], got 9"):
            evaluator.two_stage_evaluation(*head, local_scaling=mode, local_scaling_k=9, querybank=bank)
        for hubness_k in (9, -1, 129):
            with pytest.raises(ValueError, match="hubness_k must lie in|k must lie in"):
                evaluator.two_stage_evaluation(*head, local_scaling=mode, local_scaling_k=4, querybank=bank, hubness_k=hubness_k)
        with pytest.raises(ValueError, match="querybank must be"):
            evaluator.two_stage_evaluation(*head, local_scaling=mode, local_scaling_k=4, querybank=bank[:3])
        with pytest.raises(ValueError, match="memory bank is empty"):
            evaluator.two_stage_evaluation(*head, local_scaling=mode, local_scaling_k=4, querybank=(z[:0], z[:0, :, 0], z, z[..., 0]))
        with pytest.raises(ValueError, match="memory bank is empty"):              # None: the model's memory bank
            evaluator.two_stage_evaluation(_empty_bank_model(), *head[1:], local_scaling=mode, local_scaling_k=4)
        with pytest.raises(ValueError, match="nprobe=2 needs an inverted file"):
            evaluator.two_stage_evaluation(*head, local_scaling=mode, local_scaling_k=4, querybank=bank, nprobe=2)


def test_rerank_local_scaling_is_checked_by_both_eval_epochs_and_the_command_line(monkeypatch, capsys):
    from neighborretr_amd import training
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main_retrieval
    model, filled = _empty_bank_model(), _filled_bank_model()
    from_args = evaluator.rerank_local_scaling_from_args
    assert from_args(NS(), None) is None
    assert from_args(NS(rerank_local_scaling=None, rerank_top=8), None) is None
    assert from_args(NS(rerank_local_scaling="none", rerank_norm="qbnorm"), None) is None
    assert from_args(NS(rerank_local_scaling="csls", rerank_top=10), filled) == dict(local_scaling="csls", local_scaling_k=10)
    assert from_args(NS(rerank_local_scaling="ls", rerank_top=8, rerank_local_scaling_k=3, rerank_norm="none", local_scaling="nicdm",
                        local_scaling_k=50), filled) == dict(local_scaling="ls", local_scaling_k=3)          # independent of the exhaustive flags
    for eval_epoch in (lambda a: training.eval_epoch(a, model, None, "cpu"), lambda a: main_retrieval.eval_epoch(a, model, None)):
        for bad in ("is", "qbnorm", "CSLS", "mp", 1):
            with pytest.raises(ValueError, match="rerank_local_scaling must be 'csls', 'nicdm' or 'ls'"):
                eval_epoch(NS(rerank_local_scaling=bad, rerank_top=16))
        for k in (0, 129, 2.5, True):
            with pytest.raises(ValueError, match="rerank_local_scaling_k must be an integer in \\[1, 128\\]"):
                eval_epoch(NS(rerank_local_scaling="csls", rerank_top=16, rerank_local_scaling_k=k))
        for top in (0, None, 9):
            with pytest.raises(ValueError, match="needs rerank_top >= rerank_local_scaling_k = 10"):
                eval_epoch(NS(rerank_local_scaling="ls", rerank_top=top))
        with pytest.raises(ValueError, match="needs rerank_top >= rerank_local_scaling_k = 10"):
            eval_epoch(NS(rerank_local_scaling="ls"))
        with pytest.raises(ValueError, match="memory bank is empty"):              # every value fine, the bank not filled
            eval_epoch(NS(rerank_local_scaling="csls", rerank_top=16))
        with pytest.raises(ValueError, match="memory bank is empty"):
            eval_epoch(NS(rerank_local_scaling="csls", rerank_top=4, rerank_local_scaling_k=4))
    # both corrections: each is fine alone (the bank is filled), together they are refused
    for eval_epoch in (lambda a: training.eval_epoch(a, filled, None, "cpu"), lambda a: main_retrieval.eval_epoch(a, filled, None)):
        for norm in ("is", "qbnorm"):
            with pytest.raises(ValueError, match="choose one"):
                eval_epoch(NS(rerank_local_scaling="nicdm", rerank_top=16, rerank_norm=norm))

    def parse(argv):
        monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
        return main_retrieval.get_args()
    got = parse([])
    assert (got.rerank_local_scaling, got.rerank_local_scaling_k, got.rerank_norm) == ("none", 10, "none")
    assert parse(["--rerank_top", "64"]).rerank_local_scaling == "none"
    assert parse(["--rerank_local_scaling_k", "500"]).rerank_local_scaling_k == 500     # read only with the flag
    got = parse(["--rerank_top", "64", "--rerank_local_scaling", "csls"])
    assert (got.rerank_local_scaling, got.rerank_local_scaling_k, got.rerank_top) == ("csls", 10, 64)
    got = parse(["--rerank_top", "4", "--rerank_local_scaling", "ls", "--rerank_local_scaling_k", "4", "--local_scaling", "nicdm",
                 "--local_scaling_k", "7", "--rerank_lists", "8", "--rerank_probe", "2"])
    assert (got.rerank_local_scaling, got.rerank_local_scaling_k, got.local_scaling, got.local_scaling_k) == ("ls", 4, "nicdm", 7)
    for argv in (["--rerank_local_scaling", "csls"], ["--rerank_local_scaling", "csls", "--rerank_top", "9"],
                 ["--rerank_top", "8", "--rerank_local_scaling", "mp"], ["--rerank_top", "8", "--rerank_local_scaling", "qbnorm"],
                 ["--rerank_top", "64", "--rerank_local_scaling", "nicdm", "--rerank_norm", "is"],
                 ["--rerank_top", "64", "--rerank_local_scaling", "nicdm", "--rerank_local_scaling_k", "0"],
                 ["--rerank_top", "128", "--rerank_local_scaling", "nicdm", "--rerank_local_scaling_k", "129"]):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(argv)
        assert "--rerank_local_scaling" in capsys.readouterr().err


def test_labels_and_log_lines():
    assert evaluator.two_stage_local_scaling_label(64, "csls", 10) == "[two-stage C=64 QB-CSLS k=10]"
    assert evaluator.two_stage_local_scaling_label(8, "nicdm", 3) == "[two-stage C=8 QB-NICDM k=3]"
    assert evaluator.two_stage_local_scaling_label(128, "ls", 128) == "[two-stage C=128 QB-LS k=128]"
    raw = {"R1": 10.0, "R5": 50.0, "R10": None, "R50": None, "cand_recall": 75.0, "n_candidates": 8, "cols": [0]}
    label = evaluator.two_stage_local_scaling_label(8, "csls", 3)
    scaled = dict(raw, R1=20.0, mode="csls", k=3, label=label)
    lines = RetrievalMetrics.two_stage_lines(dict(raw, local_scaled=scaled), dict(raw, local_scaled=dict(scaled, MR=2.0)), "[two-stage C=8]")
    assert lines == ["Text-to-Video [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%",
                     "Video-to-Text [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%",
                     f"Text-to-Video {label}: R@1 20.0 R@5 50.0 - candidate recall 75.0%",
                     f"Video-to-Text {label}: R@1 20.0 R@5 50.0 - candidate recall 75.0% - MedR 2.0"]
    # with hubness: its lines before and after; behind the inverted file the raw lines carry the IVF tag, the scaled ones their label
    hub = RetrievalMetrics.hubness_from_occurrences([3, 0, 1], [1, 0, 1], 2, 2)
    ivf = evaluator.two_stage_ivf_label(8, 4, 2)
    t2v = dict(raw, hubness=hub, local_scaled=dict(scaled, hubness=hub))
    lines = RetrievalMetrics.two_stage_lines(t2v, t2v, ivf, ("text->video", "video->text"), " ")
    assert len(lines) == 8
    assert lines[0].startswith("text->video [two-stage C=8 IVF L=4 P=2] R@1 10.0") and lines[1].startswith(f"text->video {ivf} Hubness@2: skew")
    assert lines[4] == f"text->video {label} R@1 20.0 R@5 50.0 - candidate recall 75.0%"
    assert lines[5].startswith(f"text->video {label} Hubness@2: skew") and lines[7].startswith(f"video->text {label} Hubness@2")
    # without the new key: the lines as before
    assert RetrievalMetrics.two_stage_lines(raw, raw, "[two-stage C=8]") == lines[:0] + [
        "Text-to-Video [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%",
        "Video-to-Text [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%"]
