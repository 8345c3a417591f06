"""CPU: query-bank normalisation of two-stage retrieval without a GPU -- the restatements of
tests/rerank_norm_ref.py against hand-worked cases, and every refusal before any work: nr_cand_norm_rerank through ctypes,
ops.cand_norm_rerank, GalleryIndex, two_stage_evaluation, --rerank_norm in both eval_epochs and on the command line; the labels
and log lines."""
import ctypes
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import rerank_norm_ref as Q
from neighborretr_amd import evaluator, hip, ops, search
from neighborretr_amd.metrics import RetrievalMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ---- the restatements, by hand ------------------------------------------------------------------------------------------------------
def test_kernel_restatement_on_hand_worked_lines():
    f32 = lambda *x: np.asarray(x, dtype=np.float32)                                  # noqa: E731
    # gallery of 6; line 0: item 4 is the raw top-1 and a hub of the bank; line 1: padding, an entry past the gallery, a NaN
    cand = np.asarray([[1, 2, 4, 5], [0, 3, 9, -1], [-1, -1, -1, -1]], dtype=np.int32)
    fine = np.stack([f32(0.25, 0.25, 0.5, -0.0), f32(np.nan, 0.0, 0.75, 0.75), f32(1, 1, 1, 1)])
    norm = f32(9.0, 1.0, 2.0, -1.0, 9.0, 0.0)
    # raw: score descending, ties by lower position; absent and NaN slots never selected, although they hold the best scores
    idx, val, corr, gate = Q.cand_norm_rerank(fine, cand, 6, 3)
    assert idx.tolist() == [[4, 1, 2], [3, -1, -1], [-1, -1, -1]] and gate.tolist() == [0, 0, 0]
    assert val.tolist() == [[0.5, 0.25, 0.25], [0.0, -INF, -INF], [-INF] * 3]
    assert corr[0].tolist() == fine[0].tolist() and math.isnan(corr[1, 0]) and corr[1, 1:].tolist() == [0.0, -INF, -INF]
    assert np.all(np.isneginf(corr[2]))
    # is: beta * fine - norm[cand]; 0.25 * 4 - 1 = 0, 0.25 * 4 - 2 = -1, 0.5 * 4 - 9 = -7, -0.0 * 4 - 0 = -0.0: the hub drops to the end
    idx, val, corr, gate = Q.cand_norm_rerank(fine, cand, 6, 4, norm, None, 4.0)
    assert gate.tolist() == [1, 1, 1]
    assert corr[0].tolist() == [0.0, -1.0, -7.0, 0.0] and idx[0].tolist() == [1, 5, 2, 4] and val[0].tolist() == [0.0, 0.0, -1.0, -7.0]
    assert idx[1].tolist() == [3, -1, -1, -1] and val[1, 0] == 1.0 and math.isnan(corr[1, 0])
    assert np.all(idx[2] == -1) and np.all(np.isneginf(corr[2]))
    # qbnorm: the gate reads the raw top-1 (line 0: item 4; line 1: item 3, the only selectable slot; line 2: none)
    for active, want in (([0, 0, 0, 0, 1, 0], [1, 0, 0]), ([1, 1, 1, 0, 0, 1], [0, 0, 0]), ([0, 0, 0, 1, 0, 0], [0, 1, 0])):
        got = Q.cand_norm_rerank(fine, cand, 6, 4, norm, np.asarray(active), 4.0)
        assert got[3].tolist() == want
        assert got[0][0].tolist() == ([1, 5, 2, 4] if want[0] else [4, 1, 2, 5])
    # a tied top-1: the lower position decides, -0.0 ties with +0.0
    cand = np.asarray([[2, 3], [2, 3]], dtype=np.int32)
    fine = np.stack([f32(-0.0, 0.0), f32(0.0, -0.0)])
    assert Q.cand_norm_rerank(fine, cand, 6, 1, norm, np.asarray([0, 0, 1, 0, 0, 0]), 4.0)[3].tolist() == [1, 1]
    assert Q.cand_norm_rerank(fine, cand, 6, 1, norm, np.asarray([0, 0, 0, 1, 0, 0]), 4.0)[3].tolist() == [0, 0]
    # two roundings, not one: beta * fine is rounded to float32 before the subtraction
    x, b, c = np.float32(1 / 3), np.float32(3.0), np.float32(1.0)
    two = np.float32(np.float32(b * x) - c)
    one = np.float32(np.float64(b) * np.float64(x) - np.float64(c))
    got = Q.cand_norm_rerank(np.asarray([[x]]), np.asarray([[0]]), 1, 1, np.asarray([c]), None, 3.0)[2][0, 0]
    assert got == two == 0.0 and one != 0.0
    assert Q.same_bits([np.nan, 1.0], [-np.nan, 1.0]) and not Q.same_bits([0.0], [-0.0]) and not Q.same_bits([np.nan], [1.0])


def test_statistics_restatement_on_hand_worked_lines():
    Qm = np.asarray([[0.0, 1.0, np.nan], [0.0, -INF, np.nan], [np.nan, 1.0, np.nan]], dtype=np.float32)
    rows = Q.lse(Qm, 2.0, 1)
    assert rows[0] == pytest.approx(2.0 + math.log1p(math.exp(-2.0)), rel=1e-15) and rows[1] == 0.0 and rows[2] == 2.0
    cols = Q.lse(Qm, 2.0, 0)
    assert cols[0] == pytest.approx(math.log(2.0), rel=1e-15) and cols[1] == pytest.approx(2.0 + math.log(2.0), rel=1e-15)
    assert cols[2] == -INF                                                             # no entry left
    assert Q.lse(np.asarray([[-INF, -INF], [INF, 1.0]]), 1.0, 1).tolist() == [-INF, INF]
    # the product beta * x is a float32 product
    x = np.float32(0.1)
    assert Q.lse(np.asarray([[x]]), 20.0, 1)[0] == float(np.float32(20.0) * x) != 20.0 * float(x)
    # activation: bank items are rows (axis 1) or columns (axis 0); ties by lower index; NaN never listed
    B = np.asarray([[0.5, 0.5, 0.1, np.nan], [0.0, 0.2, 0.9, np.nan]], dtype=np.float32)
    assert Q.activation(B, 1, 1).tolist() == [True, False, True, False]
    assert Q.activation(B, 2, 1).tolist() == [True, True, True, False]
    assert Q.activation(B.T, 1, 0).tolist() == [True, False, True, False]
    assert Q.activation(B, 4, 1).tolist() == [True, True, True, False]
    occ, good = Q.occurrences(np.asarray([[0, 2], [2, -1], [2, 7]]), 3, [0, 1, 2], [1, 2, 3])
    assert occ.tolist() == [1, 0, 3] and good.tolist() == [1, 0, 1]
    rb, re_, cb, ce = Q.ground_truth(5, 2, [3, 5])
    assert (rb.tolist(), re_.tolist(), cb.tolist(), ce.tolist()) == ([0, 0, 0, 1, 1], [1, 1, 1, 2, 2], [0, 3], [3, 5])
    assert Q.topk(np.asarray([[0.1, 0.3, 0.3]], dtype=np.float32), np.asarray([[4, 6, 9]]), 10, 2).tolist() == [[6, 9]]


# ---- refusals before any work -----------------------------------------------------------------------------------------------------------
def test_nr_cand_norm_rerank_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(fine=p, cand=p, n=2, C=4, n_gallery=9, norm=p, active=p, beta=20.0, k=2, out_idx=p, out_val=p, out_corr=p, out_gate=p):
        return lib.nr_cand_norm_rerank(fine, cand, n, C, n_gallery, norm, active, beta, k, out_idx, out_val, out_corr, out_gate, None)
    for name in ("fine", "cand", "out_idx", "out_val"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("n", "n_gallery", "k"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
    assert call(C=0) == EINVAL and call(C=-1) == EINVAL and call(C=129) == EINVAL and call(C=129, k=129) == EINVAL
    assert call(k=5) == EINVAL and call(C=128, k=129) == EINVAL                        # k > C
    assert call(norm=None) == EINVAL                                                   # an activation set without normalisers
    for beta in (0.0, -1.0, float("inf"), float("nan")):
        assert call(beta=beta) == EINVAL and call(beta=beta, active=None) == EINVAL, beta
    assert hip.version() == 5 and "nr_cand_norm_rerank" in hip.exported_symbols()
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    assert "int nr_cand_norm_rerank(" in header and "#define NR_ABI_VERSION 5" in header
    args, res = hip._SIGNATURES["nr_cand_norm_rerank"]
    assert len(args) == 14 and args[7] is ctypes.c_float and res is ctypes.c_int


def test_wrapper_refuses_bad_arguments():
    fine, cand = torch.zeros((3, 4)), torch.zeros((3, 4), dtype=torch.int32)
    norm, active = torch.zeros((9,)), torch.zeros((9,), dtype=torch.int32)
    with pytest.raises(ValueError, match="must both be \\[n, C\\]"):
        ops.cand_norm_rerank(fine, cand[:, :3], 9, 2)
    with pytest.raises(ValueError, match="k must lie in"):
        ops.cand_norm_rerank(fine, cand, 9, 0)
    with pytest.raises(ValueError, match="1 <= k <= C"):
        ops.cand_norm_rerank(fine, cand, 9, 5)
    with pytest.raises(ValueError, match="1 <= k <= C"):
        ops.cand_norm_rerank(torch.zeros((3, 129)), torch.zeros((3, 129), dtype=torch.int32), 9, 2)
    with pytest.raises(ValueError, match="the gallery is empty"):
        ops.cand_norm_rerank(fine, cand, 0, 2)
    with pytest.raises(ValueError, match="needs the normalisers"):
        ops.cand_norm_rerank(fine, cand, 9, 2, active=active)
    for beta in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="beta must be finite and > 0"):
            ops.cand_norm_rerank(fine, cand, 9, 2, norm=norm, beta=beta)
    with pytest.raises(ValueError, match="norm must be a torch.float32 vector of 9"):
        ops.cand_norm_rerank(fine, cand, 9, 2, norm=norm[:8])
    with pytest.raises(ValueError, match="active must be a torch.int32 vector of 9"):
        ops.cand_norm_rerank(fine, cand, 9, 2, norm=norm, active=active.long())
    with pytest.raises(hip.NrHipError):                                                # no CPU path behind the wrapper
        ops.cand_norm_rerank(fine, cand, 9, 2, norm=norm, active=active)


def _bare_index(side="video", attached=True, n=5, d=64):
    """A GalleryIndex with nothing prepared (no GPU here): what the argument checks read, and nothing else."""
    index = object.__new__(search.GalleryIndex)
    index.model, index.side, index.query_side = None, side, "text" if side == "video" else "video"
    index.feat, index.mask = torch.zeros((n, 3, d)), torch.ones((n, 3))
    index.items = NS(n=n, n_tok=3, d=d)
    index.norm = torch.zeros((n,)) if attached else None
    index.active = torch.zeros((n,), dtype=torch.int32) if attached else None
    index.norm_beta, index.qb_k, index.n_bank = (20.0, 1, 4) if attached else (None, None, 0)
    return index


def test_index_refuses_bad_arguments_before_any_work():
    q, qm = torch.zeros((2, 3, 64)), torch.ones((2, 3))
    for mode in ("dsl", "sinkhorn", "QBNORM", "", 1, True):
        for index in (_bare_index(), _bare_index(attached=False)):
            with pytest.raises(ValueError, match="norm must be None or one of"):
                index.candidates(q, qm, 4, norm=mode)
            with pytest.raises(ValueError, match="norm must be None or one of"):
                index.search(q, qm, 2, 4, norm=mode)
    for mode in search.NORM_MODES:
        with pytest.raises(ValueError, match="attach_querybank"):
            _bare_index(attached=False).candidates(q, qm, 4, norm=mode)
        with pytest.raises(ValueError, match="attach_querybank"):
            _bare_index(attached=False).search(q, qm, 2, 4, norm=mode)
        with pytest.raises(ValueError, match="exhaustive path"):
            _bare_index().search(q, qm, 2, 0, norm=mode)
        with pytest.raises(ValueError, match="n_candidates must be an integer"):
            _bare_index().candidates(q, qm, 129, norm=mode)
        with pytest.raises(ValueError, match="1 <= k <= n_candidates"):
            _bare_index().search(q, qm, 5, 4, norm=mode)
        with pytest.raises(ValueError, match="queries are 32 wide"):
            _bare_index().search(q[..., :32], qm, 2, 4, norm=mode)
    assert search.check_norm(None) is None and search.check_norm("is") == "is" and search.NORM_MODES == ("is", "qbnorm")
    # attach_querybank: shapes, width, device, an empty bank, beta, qb_k, chunk
    index = _bare_index(attached=False)
    bank, bm = torch.zeros((4, 3, 64)), torch.ones((4, 3))
    for feat, mask, what in ((bank[0], bm, "querybank features must be"), (bank, bm[:3], "querybank mask must be"),
                             (bank, bm[:, :2], "querybank mask must be"), (bank[:0], bm[:0], "the querybank is empty"),
                             (bank[..., :32], bm, "the querybank is 32 wide, the gallery 64"),
                             (bank.to("meta"), bm.to("meta"), "same device"), (None, bm, "querybank features must be")):
        with pytest.raises(ValueError, match=what):
            index.attach_querybank(feat, mask)
    for kw, what in ((dict(beta=0.0), "beta must be finite"), (dict(beta=float("nan")), "beta must be finite"),
                     (dict(qb_k=0), "k must lie in"), (dict(qb_k=129), "k must lie in"), (dict(chunk=0), "chunk must be an integer")):
        with pytest.raises(ValueError, match=what):
            index.attach_querybank(bank, bm, **kw)
    assert index.norm is None and index.active is None and index.n_bank == 0


def _empty_bank_model():
    z = torch.zeros((0, 3, 64))
    return NS(mb_feat_t=z, mb_mask_t=z[..., 0], mb_feat_v=z, mb_mask_v=z[..., 0])


def test_two_stage_evaluation_refuses_bad_values_before_any_work():
    z = torch.zeros((4, 2, 64))
    head = (None, z, z, z[..., 0], z[..., 0], NS(world_size=1), 8)               # no model: nothing may be touched
    bank = (z, z[..., 0], z, z[..., 0])
    for mode in ("dsl", "sinkhorn", "none", 0.5):
        with pytest.raises(ValueError, match="norm must be None or one of"):
            evaluator.two_stage_evaluation(*head, norm=mode, querybank=bank)
    for beta in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="beta must be finite and > 0"):
            evaluator.two_stage_evaluation(*head, norm="is", beta=beta, querybank=bank)
    for qb_k in (0, 129):
        with pytest.raises(ValueError, match="k must lie in"):
            evaluator.two_stage_evaluation(*head, norm="qbnorm", qb_k=qb_k, querybank=bank)
    for hubness_k in (9, 128, -1, 129):
        with pytest.raises(ValueError, match="hubness_k must lie in|k must lie in"):
            evaluator.two_stage_evaluation(*head, norm="qbnorm", querybank=bank, hubness_k=hubness_k)
    with pytest.raises(ValueError, match="hubness_k must lie in"):
        evaluator.two_stage_evaluation(*head, hubness_k=9)
    with pytest.raises(ValueError, match="querybank must be"):
        evaluator.two_stage_evaluation(*head, norm="qbnorm", querybank=bank[:3])
    with pytest.raises(ValueError, match="memory bank is empty"):
        evaluator.two_stage_evaluation(*head, norm="qbnorm", querybank=(z[:0], z[:0, :, 0], z, z[..., 0]))
    with pytest.raises(ValueError, match="memory bank is empty"):                  # None: the model's memory bank
        evaluator.two_stage_evaluation(_empty_bank_model(), *head[1:], norm="is")


def test_rerank_norm_is_checked_by_both_eval_epochs_and_the_command_line(monkeypatch, capsys):
    from neighborretr_amd import training
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main_retrieval
    model = _empty_bank_model()
    assert evaluator.rerank_norm_from_args(NS(), None) is None
    assert evaluator.rerank_norm_from_args(NS(rerank_norm=None, rerank_top=8), None) is None
    assert evaluator.rerank_norm_from_args(NS(rerank_norm="none"), None) is None
    filled = NS(mb_feat_t=torch.zeros((2, 3, 64)), mb_mask_t=torch.ones((2, 3)), mb_feat_v=torch.zeros((2, 3, 64)), mb_mask_v=torch.ones((2, 3)))
    assert evaluator.rerank_norm_from_args(NS(rerank_norm="qbnorm", rerank_top=8, test_norm_beta=5.0, qb_k=3), filled) == \
        dict(norm="qbnorm", beta=5.0, qb_k=3)
    assert evaluator.rerank_norm_from_args(NS(rerank_norm="is", rerank_top=1), filled) == dict(norm="is", beta=20.0, qb_k=1)
    for eval_epoch in (lambda a: training.eval_epoch(a, model, None, "cpu"), lambda a: main_retrieval.eval_epoch(a, model, None)):
        for bad in ("dsl", "sinkhorn", "qb", 1):
            with pytest.raises(ValueError, match="rerank_norm must be 'is' or 'qbnorm'"):
                eval_epoch(NS(rerank_norm=bad, rerank_top=8))
        for top in (0, None):
            with pytest.raises(ValueError, match="needs rerank_top >= 1"):
                eval_epoch(NS(rerank_norm="qbnorm", rerank_top=top))
        with pytest.raises(ValueError, match="needs rerank_top >= 1"):
            eval_epoch(NS(rerank_norm="is"))
        with pytest.raises(ValueError, match="beta must be finite and > 0"):
            eval_epoch(NS(rerank_norm="is", rerank_top=8, test_norm_beta=0.0))
        with pytest.raises(ValueError, match="k must lie in"):
            eval_epoch(NS(rerank_norm="qbnorm", rerank_top=8, qb_k=0))
        with pytest.raises(ValueError, match="memory bank is empty"):              # every value fine, the bank not filled
            eval_epoch(NS(rerank_norm="qbnorm", rerank_top=8))

    def parse(argv):
        monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
        return main_retrieval.get_args()
    assert parse([]).rerank_norm == "none" and parse(["--rerank_top", "64"]).rerank_norm == "none"
    got = parse(["--rerank_top", "64", "--rerank_norm", "qbnorm", "--qb_k", "2", "--test_norm_beta", "10"])
    assert (got.rerank_norm, got.rerank_top, got.qb_k, got.test_norm_beta) == ("qbnorm", 64, 2, 10.0)
    assert parse(["--rerank_top", "1", "--rerank_norm", "is", "--test_norm", "dsl"]).test_norm == "dsl"      # independent flags
    for argv in (["--rerank_norm", "qbnorm"], ["--rerank_norm", "is", "--rerank_top", "0"],
                 ["--rerank_top", "8", "--rerank_norm", "dsl"], ["--rerank_top", "8", "--rerank_norm", "many"]):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(argv)
        assert "--rerank_norm" in capsys.readouterr().err


def test_labels_and_log_lines():
    assert evaluator.two_stage_norm_label(64, "qbnorm", 20.0, 1) == "[two-stage C=64 QB-Norm b=20 k=1]"
    assert evaluator.two_stage_norm_label(8, "qbnorm", 2.5, 3) == "[two-stage C=8 QB-Norm b=2.5 k=3]"
    assert evaluator.two_stage_norm_label(8, "is", 20.0, 3) == "[two-stage C=8 IS b=20]"
    raw = {"R1": 10.0, "R5": 50.0, "R10": None, "R50": None, "cand_recall": 75.0, "n_candidates": 8, "cols": [0]}
    line = RetrievalMetrics.format_two_stage(raw, prefix="text->video [two-stage C=8] ")
    assert line == "text->video [two-stage C=8] R@1 10.0 R@5 50.0 - candidate recall 75.0%"       # as before
    plain = RetrievalMetrics.two_stage_lines(raw, dict(raw, MR=2.0), "[two-stage C=8]", ("text->video", "video->text"), " ")
    assert plain == [line, "video->text [two-stage C=8] R@1 10.0 R@5 50.0 - candidate recall 75.0% - MedR 2.0"]
    label = evaluator.two_stage_norm_label(8, "qbnorm", 20.0, 1)
    hub = RetrievalMetrics.hubness_from_occurrences([3, 0, 1], [1, 0, 1], 2, 2)
    t2v = dict(raw, hubness=hub, normalised=dict(raw, R1=20.0, gated=37.5, label=label, hubness=hub))
    v2t = dict(raw, hubness=hub, normalised=dict(raw, gated=0.0, label=label, hubness=hub))
    lines = RetrievalMetrics.two_stage_lines(t2v, v2t, "[two-stage C=8]")
    assert len(lines) == 8
    assert lines[0] == "Text-to-Video [two-stage C=8]: R@1 10.0 R@5 50.0 - candidate recall 75.0%"
    assert lines[1].startswith("Text-to-Video [two-stage C=8] Hubness@2: skew") and lines[3].startswith("Video-to-Text [two-stage C=8] Hubness@2")
    assert lines[4] == f"Text-to-Video {label}: R@1 20.0 R@5 50.0 - candidate recall 75.0% - normalised 37.5% of the queries"
    assert lines[5].startswith(f"Text-to-Video {label} Hubness@2: skew")
    assert lines[6] == f"Video-to-Text {label}: R@1 10.0 R@5 50.0 - candidate recall 75.0% - normalised 0.0% of the queries"
