"""CPU: the inverted-file prefilter of two-stage retrieval without a GPU -- the restatements of tests/ivf_ref.py
against hand-worked cases, and every refusal before any work: the three nr_ivf_* entry points through ctypes, the ops wrappers,
GalleryIndex.build_ivf / candidates / search, two_stage_evaluation, --rerank_lists / --rerank_probe in both eval_epochs and on
the command line; the labels and the log line."""
import ctypes
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import ivf_ref as I
from neighborretr_amd import evaluator, hip, ops, search
from neighborretr_amd.metrics import RetrievalMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
f32 = lambda *x: np.asarray(x, dtype=np.float32)                                      # noqa: E731


# ---- the restatements, by hand ------------------------------------------------------------------------------------------------------
def test_assignment_ties_go_to_the_lower_list_and_a_zero_vector_to_list_0():
    cent = np.stack([f32(1, 0), f32(0, 1), f32(1, 0)])                                 # lists 0 and 2 have the same centroid
    x = np.stack([f32(1, 0), f32(0, 1), f32(0, 0), f32(0.6, 0.8), f32(-1, 0), f32(np.nan, 0)])
    lists = I.assign(x @ cent.T)
    # item 0 ties between lists 0 and 2 -> 0; the zero vector ties everywhere -> 0; (-1, 0) scores -1, 0, -1 -> list 1; the NaN row
    # has one selectable score (0 * nan is nan, so none at all): list 0
    assert lists.tolist() == [0, 1, 0, 1, 1, 0]
    assert I.assign(f32(-0.0, 0.0, -0.0)[None]).tolist() == [0]                        # both zeros tie
    items, offsets = I.layout(lists, 3)
    assert items.tolist() == [0, 2, 5, 1, 3, 4] and offsets.tolist() == [0, 3, 6, 6]   # ascending inside a list; list 2 is empty


def test_update_keeps_the_centroid_of_an_empty_list_and_of_a_zero_sum():
    x = np.stack([f32(1, 0), f32(-1, 0), f32(0, 1), f32(0, 1), f32(0.6, 0.8)])
    items, offsets = I.layout([0, 0, 1, 1, 1], 3)
    sums = I.list_sums(x, items, offsets)
    assert sums.tolist() == [[0.0, 0.0], [f32(0.6).item(), f32(f32(f32(1) + f32(1)) + f32(0.8)).item()], [0.0, 0.0]]
    cent = np.stack([f32(0.6, 0.8), f32(1, 0), f32(0, -1)])
    norm = np.maximum(np.linalg.norm(sums, axis=1, keepdims=True), 1e-12).astype(np.float32)
    new = I.update(cent, sums, offsets, sums / norm)
    assert new[0].tolist() == cent[0].tolist() and new[2].tolist() == cent[2].tolist()  # a zero sum; an empty list
    assert abs(float(np.linalg.norm(new[1])) - 1) < 1e-6 and new[1, 1] > new[1, 0] > 0
    # the additions are sequential float32 ones, in list order: 1 + 2^-24 + 2^-24 stays 1, the other order does not
    e = np.float32(2.0 ** -24)
    assert I.list_sums(np.asarray([[1.0], [e], [e]], dtype=np.float32), *I.layout([0, 0, 0], 1))[0, 0] == 1.0
    assert I.list_sums(np.asarray([[e], [e], [1.0]], dtype=np.float32), *I.layout([0, 0, 0], 1))[0, 0] > 1.0


def test_pool_layout_follows_the_probe_order():
    items, offsets = I.layout([2, 0, 2, 1, 0, 2], 4)                                  # lists: {1, 4}, {3}, {0, 2, 5}, {}
    assert items.tolist() == [1, 4, 3, 0, 2, 5] and offsets.tolist() == [0, 2, 3, 6, 6]
    got, base = I.pool([2, 3, 0], items, offsets)
    assert got.tolist() == [0, 2, 5, 1, 4] and base.tolist() == [0, 3, 3]             # the empty list takes no slot
    got, base = I.pool([1, -1], items, offsets)
    assert got.tolist() == [3] and base.tolist() == [0, 1]                            # a missing probe is an empty list
    got, base = I.pool([3], items, offsets)
    assert got.tolist() == [] and base.tolist() == [0]
    assert I.top_order(f32(0.5, 0.7, 0.7, np.nan), 3).tolist() == [1, 2, 0] and I.top_order(f32(np.nan), 2).tolist() == [-1, -1]


def test_selection_rule_on_hand_worked_pools():
    # ties across list boundaries and at descending item order: the lower GALLERY index wins, wherever it sits in the pool
    items = np.asarray([9, 7, 5, 3, 8, 1], dtype=np.int32)
    cand, score = I.select(f32(0.5, 0.5, 0.5, 0.5, 0.9, 0.1), items, 6, 3)
    assert cand.tolist() == [3, 5, 8] and score.tolist() == [0.5, 0.5, f32(0.9).item()]
    assert I.select(f32(0.5, 0.5, 0.5, 0.5, 0.9, 0.1), items, 4, 3)[0].tolist() == [3, 5, 7]        # only the first 4 entries
    # both zeros tie; +inf above everything, -inf below every finite score but selectable; NaN never taken
    items = np.asarray([4, 2, 6, 0, 5], dtype=np.int32)
    cand, score = I.select(f32(0.0, -0.0, np.nan, -INF, INF), items, 5, 2)
    assert cand.tolist() == [2, 5] and score.tolist()[1] == INF and np.signbit(score[0])
    cand, score = I.select(f32(0.0, -0.0, np.nan, -INF, INF), items, 5, 5)
    assert cand.tolist() == [0, 2, 4, 5, -1] and score.tolist() == [-INF, -0.0, 0.0, INF, -INF]      # pool < C: padding
    assert I.select(f32(), np.zeros(0, dtype=np.int32), 0, 2)[0].tolist() == [-1, -1]
    assert I.select(f32(np.nan, np.nan), np.asarray([1, 0]), 2, 1)[0].tolist() == [-1]
    # consequence 1: the same lists from the masked exact prefilter
    row = f32(0.3, 0.9, 0.3, 0.3, 0.8, 0.3)
    for pool_items, C in (([5, 3, 2], 2), ([5, 3, 2], 3), ([5, 3, 2], 5), ([4, 1, 0, 2, 3, 5], 4), ([], 2)):
        pool_items = np.asarray(pool_items, dtype=np.int32)
        want = I.select(row[pool_items], pool_items, len(pool_items), C)[0]
        assert I.masked_exact(row, pool_items, C).tolist() == want.tolist()
    assert I.masked_exact(row, np.asarray([5, 3, 2]), 2).tolist() == [2, 3]
    assert I.overlap([[0, 1, 2, -1], [-1, -1, -1, -1]], [[1, 2, 5, 6], [3, 4, 5, 6]]) == pytest.approx((2 / 3 + 1) / 2)


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    lib = hip.lib()
    EINVAL, EUNSUPPORTED = hip.NR_EINVAL, hip.NR_EUNSUPPORTED
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def sums(x=p, items=p, offsets=p, n_items=9, n_lists=3, d=64, out=p):
        return lib.nr_ivf_list_sums(x, items, offsets, n_items, n_lists, d, out, None)
    for name in ("x", "items", "offsets", "out"):
        assert sums(**{name: None}) == EINVAL, name
    for name in ("n_items", "n_lists", "d"):
        assert sums(**{name: 0}) == EINVAL and sums(**{name: -1}) == EINVAL, name
    assert sums(n_lists=10) == EINVAL                                                  # more lists than items

    def scan(q=p, n=5, rows=p, items=p, offsets=p, n_items=9, n_lists=3, d=64, probes=p, P=2, order=p, group=p, tiles=p, max_size=9,
             score=p, item=p, length=p, stride=9):
        return lib.nr_ivf_scan(q, n, rows, items, offsets, n_items, n_lists, d, probes, P, order, group, tiles, max_size, score, item,
                               length, stride, None)
    for name in ("q", "rows", "items", "offsets", "probes", "order", "group", "tiles", "score", "item", "length"):
        assert scan(**{name: None}) == EINVAL, name
    for name in ("n", "n_items", "n_lists", "d", "P", "stride"):
        assert scan(**{name: 0}) == EINVAL and scan(**{name: -1}) == EINVAL, name
    assert scan(n_lists=10) == EINVAL and scan(d=24) == EINVAL and scan(P=4) == EINVAL          # L > N; d % 16; P > L
    assert scan(n_items=500, n_lists=200, P=129) == EINVAL and scan(max_size=-1) == EINVAL and scan(max_size=10) == EINVAL
    assert scan(n=1 << 30, n_items=500, n_lists=200, P=128) == EUNSUPPORTED            # more than 2^31 - 1 query tiles
    assert scan(n_items=1 << 21, max_size=1 << 21) == EUNSUPPORTED                     # a list of more than 16 x 65535 rows

    def select(score=p, item=p, length=p, n=5, stride=9, C=4, cand=p, out=p):
        return lib.nr_ivf_select(score, item, length, n, stride, C, cand, out, None)
    for name in ("score", "item", "length", "cand"):
        assert select(**{name: None}) == EINVAL, name
    for name in ("n", "stride", "C"):
        assert select(**{name: 0}) == EINVAL and select(**{name: -1}) == EINVAL, name
    assert select(C=129) == EINVAL

    assert hip.version() == 5 and hip.IVF_MAX_PROBE == 128 and hip.IVF_CACHE_KEYS == 16384
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    assert "#define NR_ABI_VERSION 5" in header
    for name, n_args in (("nr_ivf_list_sums", 8), ("nr_ivf_scan", 19), ("nr_ivf_select", 9)):
        assert f"int {name}(" in header and name in hip.exported_symbols() and hasattr(lib, name)
        args, res = hip._SIGNATURES[name]
        assert len(args) == n_args and res is ctypes.c_int
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == n_args
    assert header.count("DESIGN.md 6.16") >= 4                                         # the block and each entry point cite it
    source = open(os.path.join(ROOT, "neighborretr_amd", "csrc", "nr_ivf.hip")).read()
    assert "#define NR_IVF_CACHE_KEYS 16384" in source and "DESIGN.md 6.16" in source


def test_wrappers_refuse_bad_arguments():
    items, offsets = torch.zeros((9,), dtype=torch.int32), torch.zeros((4,), dtype=torch.int32)
    x, q, probes = torch.zeros((9, 64)), torch.zeros((5, 64)), torch.zeros((5, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="list_items must be a torch.int32 vector"):
        ops.ivf_list_sums(x, items.long(), offsets)
    with pytest.raises(ValueError, match="1 <= n_lists <= n_items"):
        ops.ivf_list_sums(x, items, torch.zeros((11,), dtype=torch.int32))
    with pytest.raises(ValueError, match="x must be \\[n_items, d\\]"):
        ops.ivf_list_sums(x[:8], items, offsets)
    with pytest.raises(ValueError, match="q must be \\[n, d\\] and rows"):
        ops.ivf_scan(q[:, :32], x, items, offsets, probes, 9, 9)
    with pytest.raises(ValueError, match="probes must be a torch.int32"):
        ops.ivf_scan(q, x, items, offsets, probes.long(), 9, 9)
    with pytest.raises(ValueError, match="number of probes must lie in"):
        ops.ivf_scan(q, x, items, offsets, torch.zeros((5, 4), dtype=torch.int32), 9, 9)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.ivf_scan(q[:, :24], x[:, :24], items, offsets, probes, 9, 9)
    with pytest.raises(ValueError, match="stride >= 1"):
        ops.ivf_scan(q, x, items, offsets, probes, 0, 9)
    with pytest.raises(ValueError, match="out must be"):
        ops.ivf_scan(q, x, items, offsets, probes, 9, 9, out=(torch.zeros((5, 8)), torch.zeros((5, 9), dtype=torch.int32), items[:5]))
    score, item, length = torch.zeros((5, 9)), torch.zeros((5, 9), dtype=torch.int32), torch.zeros((5,), dtype=torch.int32)
    with pytest.raises(ValueError, match="must both be \\[n, stride\\]"):
        ops.ivf_select(score, item[:, :8], length, 4)
    with pytest.raises(ValueError, match="pool_len must be a torch.int32 vector of 5"):
        ops.ivf_select(score, item, length[:4], 4)
    for C in (0, 129):
        with pytest.raises(ValueError, match="C must lie in"):
            ops.ivf_select(score, item, length, C)
    for call in (lambda: ops.ivf_list_sums(x, items, offsets), lambda: ops.ivf_scan(q, x, items, offsets, probes, 9, 9),
                 lambda: ops.ivf_select(score, item, length, 4)):
        with pytest.raises(hip.NrHipError):                                            # no CPU path behind the wrappers
            call()


def _bare_index(n=5, d=64, n_lists=None):
    """A GalleryIndex with nothing prepared (no GPU here): what the argument checks read, and nothing else."""
    index = object.__new__(search.GalleryIndex)
    index.model, index.side, index.query_side = None, "video", "text"
    index.feat, index.mask = torch.zeros((n, 3, d)), torch.ones((n, 3))
    index.items = NS(n=n, n_tok=3, d=d, pooled=torch.zeros((n, d)))
    index.norm = index.active = index.norm_beta = index.qb_k = None
    index.n_bank = 0
    index.ivf = None if n_lists is None else NS(n_lists=n_lists)
    return index


def test_index_refuses_bad_arguments_before_any_work():
    q, qm = torch.zeros((2, 3, 64)), torch.ones((2, 3))
    index = _bare_index()
    for bad in (0, 6, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="n_lists must be an integer in \\[1, 5\\]"):
            index.build_ivf(bad)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="iters must be an integer >= 0"):
            index.build_ivf(2, iters=bad)
    for bad in (0.5, None, "0", False):
        with pytest.raises(ValueError, match="seed must be an integer"):
            index.build_ivf(2, seed=bad)
    with pytest.raises(ValueError, match="chunk must be an integer"):
        index.build_ivf(2, chunk=0)
    with pytest.raises(ValueError, match="needs a multiple of 16"):
        _bare_index(d=24).build_ivf(2)
    assert index.ivf is None
    # nprobe without an index; outside [1, min(L, 128)]; with the exhaustive path
    for call in (lambda **kw: index.candidates(q, qm, 4, **kw), lambda **kw: index.search(q, qm, 2, 4, **kw)):
        with pytest.raises(ValueError, match="call build_ivf\\(\\.\\.\\.\\) first"):
            call(nprobe=1)
    for L, bad in ((3, 0), (3, 4), (3, -1), (3, 1.0), (3, True), (300, 129)):
        built = _bare_index(n=300, n_lists=L)
        with pytest.raises(ValueError, match="nprobe must be an integer in \\[1, min\\(n_lists, 128\\)"):
            built.candidates(q, qm, 4, nprobe=bad)
        with pytest.raises(ValueError, match="nprobe must be an integer in \\[1, min\\(n_lists, 128\\)"):
            built.search(q, qm, 2, 4, nprobe=bad)
    built = _bare_index(n_lists=3)
    with pytest.raises(ValueError, match="exhaustive path \\(n_candidates = 0\\) has none"):
        built.search(q, qm, 2, 0, nprobe=2)
    with pytest.raises(ValueError, match="ivf_stats describes the inverted-file prefilter"):
        built.candidates(q, qm, 4, ivf_stats=True)
    with pytest.raises(ValueError, match="attach_querybank"):                          # norm= keeps its own checks next to nprobe
        built.search(q, qm, 2, 4, norm="is", nprobe=2)
    with pytest.raises(ValueError, match="n_candidates must be an integer"):
        built.candidates(q, qm, 129, nprobe=2)
    with pytest.raises(ValueError, match="1 <= k <= n_candidates"):
        built.search(q, qm, 5, 4, nprobe=2)
    with pytest.raises(ValueError, match="queries are 32 wide"):
        built.search(q[..., :32], qm, 2, 4, nprobe=2)
    assert search.check_nprobe(128, 500) == 128 and search.check_nprobe(3, 3) == 3
    assert search.check_ivf_build(5, 0, -7, 5) == (5, 0, -7)


def test_two_stage_evaluation_refuses_bad_values_before_any_work():
    z = torch.zeros((4, 2, 64))
    head = (None, z, z, z[..., 0], z[..., 0], NS(world_size=1), 4)                   # no model: nothing may be touched
    for bad in (-1, 2.0, "2", True):
        with pytest.raises(ValueError, match="n_lists must be an integer >= 0"):
            evaluator.two_stage_evaluation(*head, n_lists=bad, nprobe=1)
    with pytest.raises(ValueError, match="n_lists must be an integer in \\[1, 4\\]"):   # more lists than a gallery has items
        evaluator.two_stage_evaluation(*head, n_lists=5, nprobe=1)
    for bad in (0, 3, -1, None, 1.0):
        with pytest.raises(ValueError, match="nprobe must be an integer in \\[1, min\\(n_lists, 128\\) = 2\\]"):
            evaluator.two_stage_evaluation(*head, n_lists=2, nprobe=bad)
    with pytest.raises(ValueError, match="iters must be an integer >= 0"):
        evaluator.two_stage_evaluation(*head, n_lists=2, nprobe=1, ivf_iters=-1)
    with pytest.raises(ValueError, match="seed must be an integer"):
        evaluator.two_stage_evaluation(*head, n_lists=2, nprobe=1, ivf_seed=0.5)
    with pytest.raises(ValueError, match="needs an inverted file: give n_lists >= 1"):
        evaluator.two_stage_evaluation(*head, nprobe=2)


def _empty_bank_model():
    z = torch.zeros((0, 3, 64))
    return NS(mb_feat_t=z, mb_mask_t=z[..., 0], mb_feat_v=z, mb_mask_v=z[..., 0])


def test_rerank_lists_is_checked_by_both_eval_epochs_and_the_command_line(monkeypatch, capsys):
    from neighborretr_amd import training
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main_retrieval
    model = _empty_bank_model()
    assert evaluator.rerank_ivf_from_args(NS()) is None and evaluator.rerank_ivf_from_args(NS(rerank_lists=0, rerank_probe=3)) is None
    assert evaluator.rerank_ivf_from_args(NS(rerank_lists=None)) is None
    assert evaluator.rerank_ivf_from_args(NS(rerank_top=8, rerank_lists=128, rerank_probe=8)) == \
        dict(n_lists=128, nprobe=8, ivf_iters=10, ivf_seed=0)
    assert evaluator.rerank_ivf_from_args(NS(rerank_top=1, rerank_lists=4, rerank_probe=4, rerank_ivf_iters=0, rerank_ivf_seed=9)) == \
        dict(n_lists=4, nprobe=4, ivf_iters=0, ivf_seed=9)
    for eval_epoch in (lambda a: training.eval_epoch(a, model, None, "cpu"), lambda a: main_retrieval.eval_epoch(a, model, None)):
        for top in (0, None):
            with pytest.raises(ValueError, match="rerank_lists restricts the prefilter.*needs rerank_top >= 1"):
                eval_epoch(NS(rerank_lists=4, rerank_probe=2, rerank_top=top))
        with pytest.raises(ValueError, match="needs rerank_top >= 1"):
            eval_epoch(NS(rerank_lists=4, rerank_probe=2))
        for bad in (-1, 1.5, "4", True):
            with pytest.raises(ValueError, match="rerank_lists / rerank_ivf_iters / rerank_ivf_seed: n_lists must be an integer"):
                eval_epoch(NS(rerank_top=8, rerank_lists=bad, rerank_probe=1))
        for lists, bad in ((4, 0), (4, 5), (4, None), (300, 129), (4, 2.0)):
            with pytest.raises(ValueError, match="rerank_probe must be an integer in \\[1, min\\(rerank_lists, 128\\)"):
                eval_epoch(NS(rerank_top=8, rerank_lists=lists, rerank_probe=bad))
        with pytest.raises(ValueError, match="iters must be an integer >= 0"):
            eval_epoch(NS(rerank_top=8, rerank_lists=4, rerank_probe=2, rerank_ivf_iters=-1))
        with pytest.raises(ValueError, match="seed must be an integer"):
            eval_epoch(NS(rerank_top=8, rerank_lists=4, rerank_probe=2, rerank_ivf_seed=None))

    def parse(argv):
        monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
        return main_retrieval.get_args()
    got = parse([])
    assert (got.rerank_lists, got.rerank_probe, got.rerank_ivf_iters, got.rerank_ivf_seed) == (0, 0, 10, 0)
    got = parse(["--rerank_top", "64", "--rerank_lists", "128", "--rerank_probe", "8", "--rerank_ivf_iters", "3", "--rerank_ivf_seed", "5"])
    assert (got.rerank_top, got.rerank_lists, got.rerank_probe, got.rerank_ivf_iters, got.rerank_ivf_seed) == (64, 128, 8, 3, 5)
    assert parse(["--rerank_top", "8", "--rerank_lists", "300", "--rerank_probe", "128"]).rerank_probe == 128
    for argv, flag in ((["--rerank_lists", "4", "--rerank_probe", "2"], "--rerank_lists"),
                       (["--rerank_top", "8", "--rerank_lists", "-1"], "--rerank_lists"),
                       (["--rerank_top", "8", "--rerank_lists", "many"], "--rerank_lists"),
                       (["--rerank_top", "8", "--rerank_lists", "4"], "--rerank_probe"),
                       (["--rerank_top", "8", "--rerank_lists", "4", "--rerank_probe", "5"], "--rerank_probe"),
                       (["--rerank_top", "8", "--rerank_lists", "300", "--rerank_probe", "129"], "--rerank_probe"),
                       (["--rerank_top", "8", "--rerank_probe", "2"], "--rerank_probe"),
                       (["--rerank_top", "8", "--rerank_lists", "4", "--rerank_probe", "2", "--rerank_ivf_iters", "-1"], "--rerank_ivf_iters")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(argv)
        assert flag in capsys.readouterr().err


def test_labels_and_log_lines():
    assert evaluator.two_stage_ivf_label(64, 128, 8) == "[two-stage C=64 IVF L=128 P=8]"
    assert evaluator.two_stage_label(64) == "[two-stage C=64]"                         # as before
    raw = {"R1": 10.0, "R5": 50.0, "R10": None, "R50": None, "cand_recall": 75.0, "n_candidates": 8, "cols": [0]}
    tag = evaluator.two_stage_ivf_label(8, 4, 2)
    ivf = dict(raw, n_lists=4, nprobe=2, pool_mean=0.4567, ivf_overlap=0.875)
    lines = RetrievalMetrics.two_stage_lines(ivf, dict(ivf, MR=2.0), tag, ("text->video", "video->text"), " ")
    assert lines == ["text->video [two-stage C=8 IVF L=4 P=2] R@1 10.0 R@5 50.0 - candidate recall 75.0%",
                     "text->video [two-stage C=8 IVF L=4 P=2] pool 45.7% of the gallery - kept 87.5% of the exact prefilter's candidates",
                     "video->text [two-stage C=8 IVF L=4 P=2] R@1 10.0 R@5 50.0 - candidate recall 75.0% - MedR 2.0",
                     "video->text [two-stage C=8 IVF L=4 P=2] pool 45.7% of the gallery - kept 87.5% of the exact prefilter's candidates"]
    plain = RetrievalMetrics.two_stage_lines(raw, raw, "[two-stage C=8]", ("text->video", "video->text"), " ")
    assert len(plain) == 2 and not any("pool" in line for line in plain)               # without the fields: today's lines
