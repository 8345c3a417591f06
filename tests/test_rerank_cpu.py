"""CPU: two-stage retrieval without a GPU -- the fp64 restatement (tests/rerank_ref.py) against the oracle's metrics on a matrix with
planted ties, the rules that do not depend on scores, and the refusals of nr_local_level_cand, two_stage_evaluation and
--rerank_top before any work."""
import ctypes
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import nr_oracle as O
import rerank_ref as R
from neighborretr_amd import evaluator, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrix(n_rows, n_cols, seed):
    g = np.random.default_rng(seed)
    S = g.standard_normal((n_rows, n_cols)) * 0.1
    return S


def _full_lists(S):
    """Candidate lists that hold every column, ascending, with their scores."""
    cand = np.tile(np.arange(S.shape[1], dtype=np.int32), (S.shape[0], 1))
    return cand, S.copy()


def test_restatement_with_every_candidate_equals_the_oracle_metrics():
    N = 37
    S = _matrix(N, N, 1) + np.eye(N) * 0.15
    S[5, 9] = S[5, 5]               # ties with the ground truth, in a row and in a column
    S[9, 5] = S[5, 5]
    S[20, 3] = S[20, 20]
    S[11, 30] = S[30, 30]
    cand_t, fine_t = _full_lists(S)
    cand_v, fine_v = _full_lists(S.T)
    t2v, v2t = R.single_sentence(cand_t, fine_t, cand_v, fine_v, N)
    ref_t, ref_v = O.compute_metrics(S), O.compute_metrics(S.T)
    assert len(ref_t["cols"]) > N and len(ref_v["cols"]) > N        # the planted ties yield extra hits
    for got, want in ((t2v, ref_t), (v2t, ref_v)):
        assert got["cols"] == want["cols"]
        for k in ("R1", "R5", "R10", "MR", "MedianR", "MeanR"):
            assert got[k] == want[k], k
        assert got["R50"] is None and got["cand_recall"] == 100.0 and got["n_candidates"] == N
    # the product's own counting, fed the same lists, gives the same dictionaries
    gt = np.arange(N)
    for lists, want in (((cand_t, fine_t), t2v), ((cand_v, fine_v), v2t)):
        assert evaluator.two_stage_metrics(*evaluator.two_stage_counts(*lists, gt), N) == want


def test_restatement_multi_sentence_with_every_candidate_equals_the_oracle():
    sizes = [3, 1, 4, 2, 5, 1, 3]                                   # ragged groups, one-sentence groups included
    ends = np.cumsum(sizes)
    Ns, V = int(ends[-1]), len(sizes)
    S = _matrix(Ns, V, 2)
    group = np.searchsorted(ends, np.arange(Ns), side="right")
    S[np.arange(Ns), group] += 0.12
    S[4, 0] = S[4, 2]               # a sentence's own video tied with a lower and with a higher video
    S[10, 6] = S[10, 4]
    S[0, 3] = S[8, 3]               # two groups' best scores against one video tie
    cand_t = np.full((Ns, Ns), -1, dtype=np.int32)
    cand_t[:, :V] = np.arange(V)
    fine_t = np.full((Ns, Ns), -np.inf)
    fine_t[:, :V] = S
    cand_v, fine_v = _full_lists(S.T)
    t2v, v2t = R.multi_sentence(cand_t, fine_t, cand_v, fine_v, ends, Ns)
    ref_t, ref_v = O.multi_sentence_metrics(S, [int(e) - 1 for e in ends])
    for k in ("R1", "R5", "R10", "MedianR", "MR", "MeanR", "Std_Rank"):
        assert t2v[k] == ref_t[k], k
    assert t2v["R50"] is None
    assert v2t["cols"] == ref_v["cols"]
    for k in ("R1", "R5", "R10", "MR", "MeanR"):
        assert v2t[k] == ref_v[k], k
    got_t, got_v = evaluator.two_stage_multi_sentence_metrics(cand_t, fine_t, cand_v, fine_v, ends, Ns)
    assert got_t == t2v and got_v == v2t


def test_rules_that_do_not_depend_on_scores():
    # three queries, C = 6: query 1 misses its ground truth, query 2 finds it behind 5 better candidates
    cand = np.asarray([[0, 3, 4, 5, 6, 7], [0, 2, 3, 4, 5, -1], [2, 3, 4, 5, 6, 7]], dtype=np.int32)
    fine = np.asarray([[.9, .1, .2, .3, .4, .5], [.9, .8, .7, .6, .5, -np.inf], [.1, .2, .3, .4, .5, .6]])
    cnt = R.counts(cand, fine, range(3))
    assert cnt == [(True, 0, 1), (False, 0, 0), (True, 5, 1)]
    m = R.metrics(cnt, 6)
    assert m["R1"] == pytest.approx(100 / 3) and m["R5"] == pytest.approx(100 / 3)      # the missed query never counts
    assert m["R10"] is None and m["R50"] is None                                         # K > C
    assert m["cand_recall"] == pytest.approx(200 / 3) and m["cols"] == [0, 5]
    assert "MR" not in m and "MeanR" not in m and "MedianR" not in m                      # recall below 100 %
    assert evaluator.two_stage_metrics(*evaluator.two_stage_counts(cand, fine, np.arange(3)), 6) == m
    full = R.metrics([(True, 0, 1), (True, 2, 2)], 10)
    assert full["MR"] == 3.0 and full["cols"] == [0, 2, 3] and full["R10"] == 100.0 and full["R50"] is None
    # the final ordering: score descending, ties by lower gallery index, padding last
    idx, val = R.final_order(np.asarray([[1, 4, 6, -1]]), np.asarray([[.5, .7, .7, -np.inf]]), 4)
    assert idx.tolist() == [[4, 6, 1, -1]] and val.tolist() == [[.7, .7, .5, -np.inf]]
    assert R.select(np.asarray([[.1, .9, .9, .3]]), 2).tolist() == [[1, 2]]
    assert R.select(np.asarray([[.1, .9]]), 3).tolist() == [[0, 1, -1]]


def test_nr_local_level_cand_refuses_bad_arguments_before_any_launch():
    """The argument checks of nr_local_level_cand return NR_EINVAL / NR_EUNSUPPORTED on the host (no GPU needed)."""
    lib = hip.lib()
    EINVAL, EUNSUP = -1, -2
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    X3, B16 = hip.PREC_BF16X3, hip.PREC_BF16

    def call(q_hi=p, q_lo=p, g_hi=p, g_lo=p, w_q=p, w_g=p, n_q=2, Nq=24, n_g=3, Ng=12, d=512, prec=X3, cand=p, C=4, out=p):
        return lib.nr_local_level_cand(q_hi, q_lo, g_hi, g_lo, w_q, w_g, n_q, Nq, n_g, Ng, d, prec, cand, C, out, None)
    for name in ("q_hi", "g_hi", "w_q", "w_g", "cand", "out"):
        assert call(**{name: None}) == EINVAL, name
    assert call(C=0) == EINVAL and call(C=129) == EINVAL and call(C=-1) == EINVAL
    assert call(d=100) == EINVAL and call(d=0) == EINVAL
    assert call(Nq=129) == EUNSUP and call(Ng=129) == EUNSUP
    assert call(q_lo=None) == EINVAL and call(g_lo=None) == EINVAL          # split-bf16 without the lo halves
    assert call(prec=2) == EINVAL
    assert call(n_q=0) == EINVAL and call(n_g=0) == EINVAL and call(Nq=0) == EINVAL and call(Ng=0) == EINVAL
    assert call(d=2048) == EUNSUP                                            # past the zero row of absent candidates
    assert hip.version() == 5 and "nr_local_level_cand" in hip.exported_symbols()


def test_two_stage_evaluation_refuses_bad_values_before_any_work():
    z = torch.zeros((4, 2, 64))
    head = (None, z, z, z[..., 0], z[..., 0], NS(world_size=1))                  # no model: nothing may be touched
    for bad in (0, 129, -1, 2.5, "8", None, True):
        with pytest.raises(ValueError, match="n_candidates must be an integer in \\[1, 128\\]"):
            evaluator.two_stage_evaluation(*head, bad)
    for bad in (0, -3, 1.5, None):
        with pytest.raises(ValueError, match="chunk must be an integer >= 1"):
            evaluator.two_stage_evaluation(*head, 8, chunk=bad)
    with pytest.raises(ValueError, match="one text per video expected"):
        evaluator.two_stage_evaluation(None, z, z[:3], z[..., 0], z[:3, :, 0], NS(world_size=1), 8)
    with pytest.raises(ValueError, match="cut_off_points must give"):
        evaluator.two_stage_evaluation(None, z, z[:2], z[..., 0], z[:2, :, 0], NS(world_size=1), 8, cut_off_points=[1, 2])
    with pytest.raises(ValueError, match="mask \\[n, tokens\\]"):
        evaluator.two_stage_evaluation(None, z, z, z[..., 0], z[:, :1, 0], NS(world_size=1), 8)
    from neighborretr_amd import search
    with pytest.raises(ValueError, match="side must be"):
        search.GalleryIndex(None, z, z[..., 0], side="audio")
    with pytest.raises(ValueError, match="the gallery is empty"):
        search.GalleryIndex(None, z[:0], z[:0, :, 0])


def test_rerank_top_is_checked_by_both_eval_epochs_and_the_command_line(monkeypatch, capsys):
    from neighborretr_amd import training
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main_retrieval
    assert evaluator.rerank_top_from_args(NS()) == 0 and evaluator.rerank_top_from_args(NS(rerank_top=None)) == 0
    assert evaluator.rerank_top_from_args(NS(rerank_top=128)) == 128
    assert evaluator.two_stage_label(8) == "[two-stage C=8]"
    for eval_epoch in (lambda a: training.eval_epoch(a, None, None, "cpu"), lambda a: main_retrieval.eval_epoch(a, None, None)):
        for bad in (129, -1, 2.5, "8"):
            with pytest.raises(ValueError, match="rerank_top must be an integer in \\[0, 128\\]"):
                eval_epoch(NS(rerank_top=bad))

    def parse(argv):
        monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
        return main_retrieval.get_args()
    assert parse([]).rerank_top == 0 and parse(["--rerank_top", "64"]).rerank_top == 64
    for argv in (["--rerank_top", "129"], ["--rerank_top", "-1"], ["--rerank_top", "many"]):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(argv)
        assert "--rerank_top" in capsys.readouterr().err


# ---- the one gather of two_stage_evaluation: its pack / unpack pair ------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("n, W", ((5, 2), (4, 4), (1, 3)))
def test_the_gathers_pack_and_unpack_round_trip_bit_for_bit(n, W):
    """cand, fine and extras of widths 1, 2, 3 and C (and a vector, as norm's gate), packed on every rank's slice -- for (1, 3) two
    ranks own no row --, joined as _gathered_rows joins the ranks' blocks, unpacked: the unsliced tensors, every bit of them."""
    C = 6
    g = torch.Generator().manual_seed(100 * n + W)
    cand = torch.randint(-1, 40, (n, C), generator=g, dtype=torch.int32)
    cand[0, C - 1] = -1
    fine = torch.randn((n, C), generator=g)
    nans = torch.tensor([0x7FC00000, 0x7FC00001, -0x00400000 + 5, 0x7F800001], dtype=torch.int32).view(torch.float32)     # four payloads
    special = torch.cat([nans, torch.tensor([-0.0, float("-inf"), 0.0, -1.0])])

    def extra(w, dtype):
        if dtype == torch.int32:
            return torch.randint(-1, 2 ** 31 - 1, (n, w), generator=g, dtype=torch.int32)
        x = torch.randn((n, w), generator=g)
        x.view(-1)[::2] = special[torch.arange((n * w + 1) // 2) % len(special)]
        return x
    fine[0, :4], fine[n - 1, 4:] = nans, torch.tensor([-0.0, float("-inf")])
    whole = (cand, fine, extra(1, torch.float32), extra(2, torch.float32), extra(3, torch.int32), extra(C, torch.float32),
             extra(1, torch.int32)[:, 0].contiguous())
    width = -(-n // W)
    packed, specs = zip(*(evaluator._pack_rows(tuple(t[slice(*evaluator.slab_bounds(n, W, r))] for t in whole), width) for r in range(W)))
    assert all(s == specs[0] for s in specs) and [s[0] for s in specs[0]] == [C, C, 1, 2, 3, C, 1]
    assert all(p.dtype == torch.int32 and tuple(p.shape) == (2 * C + 1 + 2 + 3 + C + 1, width) for p in packed)
    rows = torch.cat([p[:, :evaluator.slab_rows(n, W, r)] for r, p in enumerate(packed)], dim=1).contiguous()
    if W == 3:
        assert [evaluator.slab_rows(n, W, r) for r in range(W)] == [1, 0, 0]
    got = evaluator._unpack_rows(rows, specs[0])
    assert len(got) == len(whole)
    for a, b in zip(got, whole):
        assert a.dtype == b.dtype and a.shape == b.shape and a.is_contiguous() and torch.equal(_bits(a), _bits(b))
    assert torch.isnan(got[1][0, :4]).all() and torch.equal(got[1][0, :4].view(torch.int32), nans.view(torch.int32))


# ---- the refusals of search.py, word for word -------------------------------------------------------------------------------------------------
def _bare_index(**attached):
    """A GalleryIndex with nothing prepared: what the argument checks read, and nothing else."""
    from neighborretr_amd import search
    index = object.__new__(search.GalleryIndex)
    index.model, index.side, index.query_side = None, "video", "text"
    index.feat, index.mask, index.items = torch.zeros((5, 3, 64)), torch.ones((5, 3)), NS(n=5, n_tok=3, d=64)
    index.norm = index.active = index.norm_beta = index.qb_k = index.ivf = index.ls_mean = index.ls_kth = index.ls_k = None
    index.n_bank = index.ls_n_bank = 0
    for name, value in attached.items():
        setattr(index, name, value)
    return index


def _refusals():
    """(id, call(search module), the message): the strings are those of the commit before the checks were folded together."""
    q, qm, z = torch.zeros((2, 3, 64)), torch.ones((2, 3)), torch.zeros((5,))
    out = []
    for bad in (True, 2.0, 0, 129, -1):
        out.append((f"candidates-{bad!r}", lambda s, bad=bad: s.check_candidates(bad), f"n_candidates must be an integer in [1, 128], got {bad!r}"))
        out.append((f"local_scaling_k-{bad!r}", lambda s, bad=bad: s.check_local_scaling_k(bad),
                    f"local scaling k must be an integer in [1, 128], got {bad!r}"))
    for bad in (False, 1.5, -1, 129):
        out.append((f"candidates0-{bad!r}", lambda s, bad=bad: s.check_candidates(bad, allow_zero=True),
                    f"n_candidates must be an integer in [0, 128], got {bad!r}"))
    for bad in (True, 8.0, 0, -2):
        out.append((f"chunk-{bad!r}", lambda s, bad=bad: s.check_chunk(bad), f"chunk must be an integer >= 1, got {bad!r}"))
    for bad in (True, 4.0, 0, 10):
        out.append((f"n_lists-{bad!r}", lambda s, bad=bad: s.check_ivf_build(bad, 10, 0, 9),
                    f"n_lists must be an integer in [1, 9] (the gallery's size), got {bad!r}"))
    for bad in (False, 1.0, -1):
        out.append((f"iters-{bad!r}", lambda s, bad=bad: s.check_ivf_build(4, bad, 0, 9), f"iters must be an integer >= 0, got {bad!r}"))
    for bad in (True, 0.0, None):
        out.append((f"seed-{bad!r}", lambda s, bad=bad: s.check_ivf_build(4, 10, bad, 9), f"seed must be an integer, got {bad!r}"))
    for bad in (True, 2.0, 0, 17):
        out.append((f"nprobe-{bad!r}", lambda s, bad=bad: s.check_nprobe(bad, 16),
                    f"nprobe must be an integer in [1, min(n_lists, 128) = 16], got {bad!r}"))
    out.append(("nprobe-200", lambda s: s.check_nprobe(129, 200), "nprobe must be an integer in [1, min(n_lists, 128) = 128], got 129"))
    out.append(("norm-mode", lambda s: s.check_norm("dsl"), "norm must be None or one of ('is', 'qbnorm'), got 'dsl'"))
    out.append(("local_scaling-mode", lambda s: s.check_local_scaling("mp"),
                "local_scaling must be None or one of ('csls', 'nicdm', 'ls'), got 'mp'"))
    for how in ("candidates", "search"):
        def call(index, how=how, **kw):
            return index.candidates(q, qm, kw.pop("C", 4), **kw) if how == "candidates" else index.search(q, qm, 2, kw.pop("C", 4), **kw)
        out.append((f"{how}-k" if how == "search" else f"{how}-ivf_stats",
                    (lambda s: _bare_index().search(q, qm, True, 4)) if how == "search" else (lambda s: _bare_index().candidates(q, qm, 4, ivf_stats=True)),
                    "k must be an integer in [1, 4] (1 <= k <= n_candidates), got True" if how == "search" else
                    "ivf_stats describes the inverted-file prefilter: it needs nprobe"))
        out.append((f"{how}-no-ivf", lambda s, call=call: call(_bare_index(), nprobe=2),
                    "nprobe=2 needs the gallery's inverted file: call build_ivf(...) first"))
        out.append((f"{how}-no-querybank", lambda s, call=call: call(_bare_index(ls_mean=z, ls_kth=z, ls_k=2), norm="is"),
                    "norm='is' needs the gallery's query-bank statistics: call attach_querybank(...) first"))
        out.append((f"{how}-no-localscale", lambda s, call=call: call(_bare_index(norm=z), local_scaling="csls"),
                    "local_scaling='csls' needs the gallery's neighbourhood statistics: call attach_localscale(...) first"))
        out.append((f"{how}-both", lambda s, call=call: call(_bare_index(norm=z, ls_mean=z, ls_kth=z, ls_k=2), norm="qbnorm", local_scaling="ls"),
                    "local_scaling='ls' and norm='qbnorm' both correct the candidate scores: choose one"))
        out.append((f"{how}-too-few", lambda s, call=call: call(_bare_index(ls_mean=z, ls_kth=z, ls_k=3), C=2, local_scaling="nicdm"),
                    "local_scaling takes a query's neighbourhood of ls_k = 3 among its candidates: n_candidates >= 3 expected, got 2"))
    for name in ("norm", "local_scaling"):
        out.append((f"search-exhaustive-{name}",
                    lambda s, name=name: _bare_index(norm=z, ls_mean=z, ls_kth=z, ls_k=2).search(q, qm, 2, 0, **{name: "is" if name == "norm" else "ls"}),
                    f"{name} acts on candidate lists: the exhaustive path (n_candidates = 0) has the evaluator's corrections"))
    out.append(("search-exhaustive-nprobe", lambda s: _bare_index(ivf=NS(n_lists=4)).search(q, qm, 2, 0, nprobe=2),
                "nprobe restricts the prefilter: the exhaustive path (n_candidates = 0) has none"))
    return out


@pytest.mark.parametrize("call, message", [pytest.param(c, m, id=i) for i, c, m in _refusals()])
def test_search_refusals_keep_their_wording(call, message):
    from neighborretr_amd import search
    with pytest.raises(ValueError) as e:
        call(search)
    assert str(e.value) == message
