"""CPU: the NumPy restatement of IS, DSL and QB-Norm (hubnorm_ref) on hand-worked matrices with a planted hub column, the
host-side refusals of the nr_hubnorm_* entry points, and the command-line flags."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import hubnorm_ref as R
from neighborretr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA = 20.0

# 3 texts x 3 videos: video 2 is a hub -- every text scores it high, texts 0 and 1 even above their own video
S3 = np.array([[0.50, 0.10, 0.60],
               [0.20, 0.45, 0.55],
               [0.05, 0.15, 0.70]], dtype=np.float32)
# 4 texts x 5 videos: video 1 is the hub
S45 = np.array([[0.40, 0.62, 0.10, 0.05, 0.20],
                [0.12, 0.64, 0.50, 0.10, 0.15],
                [0.05, 0.61, 0.20, 0.55, 0.10],
                [0.15, 0.60, 0.05, 0.25, 0.45]], dtype=np.float32)


def test_lse_follows_the_definition_by_hand():
    x = np.array([[0.1, np.nan, 0.3], [np.nan, np.nan, np.nan], [-np.inf, -np.inf, np.nan], [np.inf, 0.0, 1.0]], np.float32)
    got = R.lse(x, 2.0, 1)
    b = np.float32(2.0) * x.astype(np.float32)
    assert got[0] == pytest.approx(np.log(np.exp(float(b[0, 0])) + np.exp(float(b[0, 2]))), rel=1e-15)
    assert got[1] == -np.inf                                   # no entry left
    assert got[2] == -np.inf                                   # max -inf: -inf + log 2
    assert got[3] == np.inf                                    # an entry equal to the max adds exactly 1
    assert np.array_equal(R.lse(x.T, 2.0, 0), got)


@pytest.mark.parametrize("S,hub", [(S3, 2), (S45, 1)])
def test_is_lowers_the_hub_against_the_other_columns(S, hub):
    T, V = R.normalise(S, "is", BETA)
    assert T.dtype == np.float32
    others = [j for j in range(S.shape[1]) if j != hub]
    # per text row: the gap hub - best other column shrinks (the hub's normaliser is the largest)
    c_v = R.lse(S, BETA, 0)
    assert c_v[hub] > c_v[others].max()
    for i in range(S.shape[0]):
        raw_gap = BETA * (S[i, hub] - S[i, others].max())
        assert T[i, hub] - T[i, others].max() < raw_gap
    # the hub loses top-1 slots: fewer text rows have it as their best video
    assert np.sum(T.argmax(1) == hub) < np.sum(S.argmax(1) == hub)
    # V: per-row shift only, so every video's ranking of the texts is the raw one shifted -- checked bitwise by definition
    want = (np.float32(BETA) * S - R.lse(S, BETA, 1).astype(np.float32)[:, None]).astype(np.float32)
    assert np.array_equal(V.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("S", [S3, S45])
def test_dsl_equals_torch_dual_softmax(S):
    T, V = R.normalise(S, "dsl", BETA)
    St = torch.from_numpy(S).double()
    b = float(np.float32(BETA))
    want_t = St * torch.softmax(b * St, dim=0)                 # text->video: the texts are the query axis of each video column
    want_v = St * torch.softmax(b * St, dim=1)                 # video->text: the videos are the query axis of each text row
    assert np.allclose(T, want_t.numpy(), rtol=1e-6, atol=0)
    assert np.allclose(V, want_v.numpy(), rtol=1e-6, atol=0)


def _bank_for(S, rng_seed=0):
    rng = np.random.default_rng(rng_seed)
    Qt = rng.uniform(-0.2, 0.8, (6, S.shape[1])).astype(np.float32)
    Qv = rng.uniform(-0.2, 0.8, (S.shape[0], 7)).astype(np.float32)
    return Qt, Qv


@pytest.mark.parametrize("S", [S3, S45])
def test_qbnorm_with_every_query_gated_is_is_with_the_bank_statistics(S):
    Qt, Qv = _bank_for(S)
    qb_k = max(S.shape)                                        # every gallery item is active
    row_gate, col_gate = R.gates(S, Qt, Qv, qb_k)
    assert row_gate.all() and col_gate.all()
    T, V = R.normalise(S, "qbnorm", BETA, Qt, Qv, qb_k)
    want_t = R.is_scores(S, BETA, R.lse(Qt, BETA, 0), 0)
    want_v = R.is_scores(S, BETA, R.lse(Qv, BETA, 1), 1)
    assert np.array_equal(T.view(np.uint32), want_t.view(np.uint32))
    assert np.array_equal(V.view(np.uint32), want_v.view(np.uint32))


@pytest.mark.parametrize("S", [S3, S45])
def test_qbnorm_with_no_query_gated_is_s(S):
    n, N = S.shape
    # every bank text prefers a video that is no text's top-1; every bank video a text that is no video's top-1, or (S3:
    # each text is some video's top-1) the bank videos have no score at all, so A_t is empty
    free_v = [j for j in range(N) if j not in set(S.argmax(1))]
    free_t = [i for i in range(n) if i not in set(S.argmax(0))]
    Qt = np.zeros((4, N), np.float32)
    Qt[:, free_v[0]] = 1.0
    Qv = np.full((n, 3), np.nan, np.float32)
    if free_t:
        Qv[:] = 0.0
        Qv[free_t[0], :] = 1.0
    row_gate, col_gate = R.gates(S, Qt, Qv, 1)
    assert not row_gate.any() and not col_gate.any()
    T, V = R.normalise(S, "qbnorm", BETA, Qt, Qv, 1)
    assert np.array_equal(T, S) and np.array_equal(V, S)


def test_qbnorm_gates_exactly_the_queries_whose_top1_is_active():
    S = S45
    Qt = np.zeros((3, 5), np.float32)
    Qt[:, 1] = 1.0                                             # A_v = {1}: the hub
    Qv = np.zeros((4, 2), np.float32)
    Qv[2, :] = 1.0                                             # A_t = {2}
    row_gate, col_gate = R.gates(S, Qt, Qv, 1)
    assert row_gate.tolist() == [True, True, True, True]       # every text's top-1 is the hub
    assert col_gate.tolist() == (S.argmax(0) == 2).tolist()
    T, V = R.normalise(S, "qbnorm", BETA, Qt, Qv, 1)
    assert np.array_equal(V[:, ~col_gate], S[:, ~col_gate])
    assert np.array_equal(T, R.is_scores(S, BETA, R.lse(Qt, BETA, 0), 0))


def test_reference_ranks_follow_the_tie_rules():
    M = np.array([[1.0, 1.0, 0.5], [2.0, 1.0, 1.0], [0.0, 0.0, 0.0]], np.float32)
    assert R.single_ranks(M).tolist() == [0, 1, 1, 2, 0, 1, 2]
    T = np.array([[0.5, 0.5], [0.7, 0.2], [np.nan, 0.3]], np.float32)        # sentences {0, 1} -> video 0, {2} -> video 1
    assert R.group_ranks(T, [1, 2]).tolist() == [0, 0, 1]
    want = np.array([[0.7, -np.inf], [0.5, 0.3]], np.float32).astype(np.float64)
    assert np.array_equal(R.group_max(T, [1, 2]), want)


# ---- entry points ------------------------------------------------------------------------------------------------------
NAMES = ("nr_hubnorm_row_lse", "nr_hubnorm_col_workspace", "nr_hubnorm_col_stats", "nr_hubnorm_combine", "nr_hubnorm_apply")


def test_hubnorm_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    for name in NAMES:
        assert (f"int {name}(" in header or f"size_t {name}(" in header) and name in hip.exported_symbols()
        assert hasattr(hip.lib(), name)
    assert hip.ABI_VERSION == 5 and hip.version() == 5


def test_hubnorm_entry_points_refuse_bad_arguments_before_any_launch():
    lib = hip.lib()                                            # host-side checks: no device needed
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    IS, DSL = hip.HUBNORM_IS, hip.HUBNORM_DSL
    for beta in (0.0, -1.0, float("inf"), float("nan"), -float("inf")):
        assert lib.nr_hubnorm_row_lse(p, 4, 8, beta, p, None) == EINVAL
        assert lib.nr_hubnorm_col_stats(p, 4, 8, beta, p, p, None) == EINVAL
        assert lib.nr_hubnorm_apply(p, 4, 8, beta, IS, p, None, p, p, None, p, None) == EINVAL
    # null pointers
    assert lib.nr_hubnorm_row_lse(None, 4, 8, 20.0, p, None) == EINVAL
    assert lib.nr_hubnorm_row_lse(p, 4, 8, 20.0, None, None) == EINVAL
    assert lib.nr_hubnorm_col_stats(None, 4, 8, 20.0, p, p, None) == EINVAL
    assert lib.nr_hubnorm_col_stats(p, 4, 8, 20.0, None, p, None) == EINVAL
    assert lib.nr_hubnorm_col_stats(p, 4, 8, 20.0, p, None, None) == EINVAL
    assert lib.nr_hubnorm_combine(2, None, 8, p, p, None) == EINVAL
    assert lib.nr_hubnorm_combine(2, p, 8, None, None, None) == EINVAL
    assert lib.nr_hubnorm_apply(None, 4, 8, 20.0, IS, p, None, p, p, None, p, None) == EINVAL
    assert lib.nr_hubnorm_apply(p, 4, 8, 20.0, IS, p, None, None, p, None, None, None) == EINVAL     # no output
    assert lib.nr_hubnorm_apply(p, 4, 8, 20.0, IS, None, None, p, p, None, p, None) == EINVAL        # T without col_norm
    assert lib.nr_hubnorm_apply(p, 4, 8, 20.0, DSL, p, None, p, None, None, p, None) == EINVAL       # V without row_norm
    # unknown mode
    for mode in (-1, 2, 7):
        assert lib.nr_hubnorm_apply(p, 4, 8, 20.0, mode, p, None, p, p, None, p, None) == EINVAL
    # negative extents
    assert lib.nr_hubnorm_row_lse(p, -1, 8, 20.0, p, None) == EINVAL
    assert lib.nr_hubnorm_row_lse(p, 4, -8, 20.0, p, None) == EINVAL
    assert lib.nr_hubnorm_col_stats(p, -4, 8, 20.0, p, p, None) == EINVAL
    assert lib.nr_hubnorm_col_stats(p, 4, -1, 20.0, p, p, None) == EINVAL
    assert lib.nr_hubnorm_combine(-1, p, 8, p, p, None) == EINVAL
    assert lib.nr_hubnorm_combine(2, p, -8, p, p, None) == EINVAL
    assert lib.nr_hubnorm_apply(p, -4, 8, 20.0, IS, p, None, p, p, None, p, None) == EINVAL
    assert lib.nr_hubnorm_apply(p, 4, -8, 20.0, IS, p, None, p, p, None, p, None) == EINVAL
    # the workspace query: ceil(n / 64) pairs of L floats, nothing for an empty or negative extent
    assert lib.nr_hubnorm_col_workspace(130, 10) == 3 * 2 * 10 * 4
    assert lib.nr_hubnorm_col_workspace(0, 10) == 0 and lib.nr_hubnorm_col_workspace(-3, 10) == 0
    assert lib.nr_hubnorm_col_workspace(5, -1) == 0


def test_ops_refuse_bad_arguments_on_the_host():
    from neighborretr_amd import evaluator, ops
    for beta in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops._check_beta(beta)
    for mode, qb_k, hk in (("ISX", 1, 0), ("is", 0, 0), ("qbnorm", 129, 0), ("dsl", 1, 129)):
        with pytest.raises(ValueError):
            evaluator._check_test_norm(mode, 20.0, qb_k, hk)
    with pytest.raises(ValueError, match="load_memory_bank"):
        e, em = torch.empty((0, 0, 0)), torch.empty((0, 0))
        evaluator._querybank(type("M", (), dict(mb_feat_t=e, mb_feat_v=e, mb_mask_t=em, mb_mask_v=em))(), None, "cpu")


def _parse(argv, monkeypatch):
    sys.path.insert(0, ROOT)
    import main_retrieval
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
    return main_retrieval.get_args()


def test_main_retrieval_accepts_the_test_norm_flags(monkeypatch):
    a = _parse([], monkeypatch)
    assert a.test_norm == "none" and a.test_norm_beta == 20.0 and a.qb_k == 1
    a = _parse(["--test_norm", "qbnorm", "--test_norm_beta", "12.5", "--qb_k", "3"], monkeypatch)
    assert a.test_norm == "qbnorm" and a.test_norm_beta == 12.5 and a.qb_k == 3
    for mode in ("is", "dsl"):
        assert _parse(["--test_norm", mode], monkeypatch).test_norm == mode


def test_main_retrieval_rejects_an_unknown_mode(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(["--test_norm", "csls"], monkeypatch)
