"""GPU: test-time hubness reduction (neighborretr_amd/csrc/nr_hubnorm.hip, evaluator.sharded_normalised_*).

The statistics kernels against the fp64 restatement (hubnorm_ref) on awkward shapes with NaN lines, infinities and signed
zeros; the cross-rank combine; the apply kernel bit for bit (IS) and to 2e-6 (DSL) given the GPU's own normalisers; the
sharded evaluator under emulated ranks and two gloo ranks, single- and multi-sentence; that IS and DSL do reduce a planted
hub and that QB-Norm normalises exactly the queries it should; eval_epoch and main_retrieval.py with and without the flag."""
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hubnorm_ref as R
import hubness_ref as H
from neighborretr_amd import comm, evaluator, modeling, ops, synth, training
from util import golden, params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BETA = 20.0
N, Nt, Nv = 96, 24, 12
MODES = ("is", "dsl", "qbnorm")


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _close(got, want, rtol):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want, rtol=rtol, atol=rtol)


def _planted(n, L, seed):
    rng = np.random.default_rng(seed)
    S = (np.round(rng.standard_normal((n, L)) * 8) / 32).astype(np.float32)
    flat = S.reshape(-1)
    for val, frac in ((0.0, 0.05), (-0.0, 0.05), (np.inf, 0.005), (-np.inf, 0.02), (np.nan, 0.05)):
        at = rng.choice(flat.size, max(1, int(frac * flat.size)), replace=False)
        flat[at] = val
    if n > 2:
        S[0] = np.nan                                         # a row that is entirely NaN
        S[1, :] = -np.inf                                     # a row of -inf only
    if L > 3:
        S[:, 2] = np.nan                                      # a column that is entirely NaN
        S[:, 3] = 0.0
        S[::2, 3] = -0.0                                      # a column of signed zeros only
    return S


# ---- 1. row and column statistics -----------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 37), (130, 129), (90, 1000), (3, 20000)]


@pytest.mark.parametrize("n,L", SHAPES)
def test_row_and_column_statistics_equal_the_definition(n, L):
    S = _planted(n, L, 7 * n + L)
    St = torch.from_numpy(S).to(DEV)
    row = ops.hubnorm_row_lse(St, BETA)
    stats = ops.hubnorm_col_stats(St, BETA)
    col = ops.hubnorm_combine(stats[None])
    _close(row.cpu().numpy(), R.lse(S, BETA, 1), 1e-6)
    _close(col.cpu().numpy(), R.lse(S, BETA, 0), 1e-6)
    # a second run gives the same bits
    assert _same_bits(ops.hubnorm_row_lse(St, BETA).cpu().numpy(), row.cpu().numpy())
    assert _same_bits(ops.hubnorm_col_stats(St, BETA).cpu().numpy(), stats.cpu().numpy())
    # a misaligned slab (the scalar paths) agrees with the definition too
    if L % 4 == 0 and n > 1:
        Sm = torch.empty(n * L + 1, device=DEV)[1:].view(n, L)
        Sm.copy_(St)
        _close(ops.hubnorm_row_lse(Sm, BETA).cpu().numpy(), R.lse(S, BETA, 1), 1e-6)
        _close(ops.hubnorm_combine(ops.hubnorm_col_stats(Sm, BETA)[None]).cpu().numpy(), R.lse(S, BETA, 0), 1e-6)


def test_statistics_of_an_empty_slab():
    S = torch.empty((0, 17), device=DEV)
    stats = ops.hubnorm_col_stats(S, BETA)
    assert torch.all(stats[0] == float("-inf")) and torch.all(stats[1] == 0)
    assert torch.all(ops.hubnorm_combine(stats[None]) == float("-inf"))
    assert ops.hubnorm_row_lse(S, BETA).numel() == 0


# ---- 2. cross-rank combine --------------------------------------------------------------------------------------------------
def _emulated(W, fn):
    world = comm.EmulatedWorld(W, real_collectives=False)
    out = {}

    def run(r):
        c = world.comm(r)
        with comm.use(c):
            c.begin_step()
            out[r] = fn(SimpleNamespace(world_size=W), r)
    world.settle(run)
    return [out[r] for r in range(W)]


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_column_statistics_of_row_splits_combine_to_the_whole(W):
    S = _planted(101, 67, 31 + W)
    St = torch.from_numpy(S).to(DEV)
    whole = ops.hubnorm_combine(ops.hubnorm_col_stats(St, BETA)[None]).cpu().numpy()

    def fn(a, r):
        r0, r1 = evaluator.slab_bounds(S.shape[0], W, r)
        return evaluator._gathered_lse(ops.hubnorm_col_stats(St[r0:r1].contiguous(), BETA), W).cpu().numpy()
    outs = _emulated(W, fn)
    for o in outs:
        assert _same_bits(o, outs[0])                         # every rank holds the same bits
    _close(outs[0], whole.astype(np.float64), 1e-6)
    _close(outs[0], R.lse(S, BETA, 0), 1e-6)


# ---- 3. apply ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(3, 37), (130, 129), (90, 1000)])
def test_apply_is_bit_exact_and_dsl_close(n, L):
    rng = np.random.default_rng(n + L)
    S = rng.uniform(-1, 1, (n, L)).astype(np.float32)
    S[0, :3] = [0.0, -0.0, np.nan]
    St = torch.from_numpy(S).to(DEV)
    c_v = ops.hubnorm_combine(ops.hubnorm_col_stats(St, BETA)[None])
    c_t = ops.hubnorm_row_lse(St, BETA)
    cv, ct = c_v.cpu().numpy(), c_t.cpu().numpy()
    T, V = ops.hubnorm_apply(St, BETA, "is", col_norm=c_v, row_norm=c_t)
    assert _same_bits(T.cpu().numpy(), R.is_scores(S, BETA, cv, 0))
    assert _same_bits(V.cpu().numpy(), R.is_scores(S, BETA, ct, 1))
    T, V = ops.hubnorm_apply(St, BETA, "dsl", col_norm=c_v, row_norm=c_t)
    for got, want in ((T, R.dsl_scores(S, BETA, cv, 0)), (V, R.dsl_scores(S, BETA, ct, 1))):
        got = got.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        np.testing.assert_allclose(got[ok], want[ok], rtol=2e-6, atol=0)
    # gates switch exactly the stated rows (T) and columns (V); one output alone
    rg = torch.from_numpy((np.arange(n) % 3 == 1).astype(np.int32)).to(DEV)
    cg = torch.from_numpy((np.arange(L) % 4 == 2).astype(np.int32)).to(DEV)
    T, V = ops.hubnorm_apply(St, BETA, "is", col_norm=c_v, row_gate=rg, row_norm=c_t, col_gate=cg)
    T, V = T.cpu().numpy(), V.cpu().numpy()
    want_t = np.where(rg.cpu().numpy()[:, None] != 0, R.is_scores(S, BETA, cv, 0), S)
    want_v = np.where(cg.cpu().numpy()[None, :] != 0, R.is_scores(S, BETA, ct, 1), S)
    assert _same_bits(T, want_t) and _same_bits(V, want_v)
    T1, V1 = ops.hubnorm_apply(St, BETA, "is", col_norm=c_v, row_gate=rg, want_v=False)
    assert V1 is None and _same_bits(T1.cpu().numpy(), want_t)


# ---- 4. the sharded evaluator --------------------------------------------------------------------------------------------
def _model():
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    return m.to(DEV).eval()


def _testset(n=N, seed=4242):
    t, v, tm, vm = synth.make_samples(seed, "test", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, v, tm.astype(np.float32), vm.astype(np.float32)))


def _bank(n=40, seed=77):
    t, v, tm, vm = synth.make_samples(seed, "train", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, tm.astype(np.float32), v, vm.astype(np.float32)))


def _full(m, a, b, am, bm, W):
    n = a.shape[0]
    return np.concatenate([evaluator._slab_similarity(m, a, b, am, bm, *evaluator.slab_bounds(n, W, r)).cpu().numpy()
                           for r in range(W)])


def _ref_metrics(T, V, cut=None):
    if cut is None:
        return R.single_ranks(T), R.single_ranks(V.T)
    return R.group_ranks(T, cut), R.single_ranks(R.group_max(V, cut))


def _same_metrics(a, b):
    assert set(a) == set(b)
    for key in a:
        if key == "hubness":
            for hk in a[key]:
                if isinstance(a[key][hk], np.ndarray):
                    assert np.array_equal(a[key][hk], b[key][hk]), hk
                else:
                    assert a[key][hk] == b[key][hk], hk
        else:
            assert a[key] == b[key], key


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_evaluator_under_emulated_ranks_equals_the_restatement(mode, W):
    m = _model()
    t, v, tm, vm = _testset()
    bank = _bank() if mode == "qbnorm" else None

    def fn(a, r):
        slabs = evaluator.sharded_normalised_slabs(m, t, v, tm, vm, a, mode, BETA, querybank=bank, qb_k=2)
        met = evaluator.sharded_normalised_metrics(m, t, v, tm, vm, a, mode, BETA, querybank=bank, qb_k=2, hubness_k=5)
        return tuple(x.cpu().numpy() for x in slabs), met
    outs = _emulated(W, fn)
    T = np.concatenate([o[0][0] for o in outs])
    V = np.concatenate([o[0][1] for o in outs])
    for _, met in outs:
        _same_metrics(met[0], outs[0][1][0])
        _same_metrics(met[1], outs[0][1][1])
    t2v, v2t = outs[0][1]
    rt, rv = _ref_metrics(T, V)
    assert t2v["cols"] == rt.tolist() and v2t["cols"] == rv.tolist()
    assert t2v["mode"] == mode and t2v["beta"] == BETA
    ht, hv = H.hubness(T, 5)[0], H.hubness(V, 5)[1]
    assert np.array_equal(t2v["hubness"]["occurrence"], ht["occ"])
    assert np.array_equal(v2t["hubness"]["occurrence"], hv["occ"])
    # the slabs against the definitions, from the same split's S
    S = _full(m, t, v, tm, vm, W)
    if mode == "qbnorm":
        Qt = _full(m, bank[0], v, bank[1], vm, W)
        Qv = _full(m, t, bank[2], tm, bank[3], W)
        rg, cg = R.gates(S, Qt, Qv, 2)
        assert np.array_equal(T[~rg], S[~rg]) and np.array_equal(V[:, ~cg], S[:, ~cg])
        _close(T[rg], R.normalise(S, "qbnorm", BETA, Qt, Qv, 2)[0][rg], 1e-5)
    else:
        Tr, Vr = R.normalise(S, mode, BETA)
        _close(T, Tr, 1e-5)
        _close(V, Vr, 1e-5)


def _margin_ok(M, tol=1e-4):
    """No rank-deciding pair (a query's own score against another) within a relative tol."""
    M = np.asarray(M, dtype=np.float64)
    d = np.diag(M)[:, None]
    gap = np.abs(M - d) / np.maximum(np.maximum(np.abs(M), np.abs(d)), 1e-30)
    np.fill_diagonal(gap, np.inf)
    return bool(gap.min() > tol)


@pytest.mark.parametrize("mode", ("is", "dsl"))
def test_recall_equals_the_fp64_restatement_on_a_well_separated_set(mode):
    m = _model()
    n = 48
    for seed in range(100, 140):
        t, v, tm, vm = _testset(n, seed)
        S = _full(m, t, v, tm, vm, 1)
        Tr, Vr = R.normalise(S, mode, BETA)
        if _margin_ok(Tr) and _margin_ok(Vr.T):
            break
    assert _margin_ok(Tr) and _margin_ok(Vr.T), "no well-separated seeded set found"
    rt, rv = _ref_metrics(Tr, Vr)
    for W in (1, 2, 3):
        t2v, v2t = _emulated(W, lambda a, r: evaluator.sharded_normalised_metrics(m, t, v, tm, vm, a, mode, BETA))[0]
        for k in (1, 5, 10):
            assert t2v[f"R{k}"] == R.recall(rt, k) and v2t[f"R{k}"] == R.recall(rv, k), (W, k)


@pytest.mark.parametrize("mode", MODES)
def test_multi_sentence_fixture_under_emulated_ranks(mode):
    g = golden("multi_sentence")
    S, cut = g["S"].astype(np.float32), g["cut_off_points"].tolist()
    Ns, V_ = S.shape
    ends = np.asarray(cut, dtype=np.int64) + 1
    St = torch.from_numpy(S).to(DEV)
    rng = np.random.default_rng(3)
    Qt_full = torch.from_numpy(rng.uniform(-1, 1, (9, V_)).astype(np.float32)).to(DEV)
    Qv_full = torch.from_numpy(rng.uniform(-1, 1, (Ns, 11)).astype(np.float32)).to(DEV)
    for W in (1, 2, 3):
        def fn(a, r, W=W):
            r0, r1 = evaluator.slab_bounds(Ns, W, r)
            q0, q1 = evaluator.slab_bounds(9, W, r)
            bank = (Qt_full[q0:q1].contiguous(), Qv_full[r0:r1].contiguous()) if mode == "qbnorm" else None
            T, V = evaluator._normalised_from_slab(St[r0:r1].contiguous(), Ns, V_, W, r, mode, BETA, bank, 1)
            met = evaluator._metrics_from_normalised(T, V, Ns, V_, W, r, ends, 3)
            return T.cpu().numpy(), V.cpu().numpy(), met
        outs = _emulated(W, fn)
        T = np.concatenate([o[0] for o in outs])
        Vn = np.concatenate([o[1] for o in outs])
        for o in outs:
            _same_metrics(o[2][0], outs[0][2][0])
            _same_metrics(o[2][1], outs[0][2][1])
        t2v, v2t = outs[0][2]
        rt, rv = _ref_metrics(T, Vn, cut)
        want_t = training.RetrievalMetrics.multi_sentence_metrics_from_ranks(rt)
        want_v = training.RetrievalMetrics.metrics_from_ranks(rv)
        for key in ("R1", "R5", "R10", "MedianR", "MeanR"):
            assert t2v[key] == want_t[key] and v2t[key] == want_v[key], (W, key)
        if mode == "qbnorm":
            Tr, Vr = R.normalise(S, mode, BETA, Qt_full.cpu().numpy(), Qv_full.cpu().numpy(), 1)
        else:
            Tr, Vr = R.normalise(S, mode, BETA)
        _close(T, Tr, 1e-5)
        _close(Vn, Vr, 1e-5)


# ---- 5. two gloo ranks ------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    args = SimpleNamespace(world_size=world, local_rank=rank)
    m = _model()
    t, v, tm, vm = _testset()
    res = {mode: evaluator.sharded_normalised_metrics(m, t, v, tm, vm, args, mode, BETA, querybank=_bank(), hubness_k=5)
           for mode in ("dsl", "qbnorm")}
    torch.save(res, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_a_single_process(tmp_path):
    import torch.multiprocessing as mp
    m = _model()
    t, v, tm, vm = _testset()
    world, port = 2, 29671
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    want = {mode: _emulated(world, lambda a, r, mode=mode: evaluator.sharded_normalised_metrics(
        m, t, v, tm, vm, a, mode, BETA, querybank=_bank(), hubness_k=5))[0] for mode in ("dsl", "qbnorm")}
    one = {mode: evaluator.sharded_normalised_metrics(m, t, v, tm, vm, SimpleNamespace(world_size=1), mode, BETA,
                                                      querybank=_bank(), hubness_k=5) for mode in ("dsl", "qbnorm")}
    for r in range(world):
        res = torch.load(f"{out}.{r}", weights_only=False)
        for mode in ("dsl", "qbnorm"):
            for d in range(2):
                _same_metrics(res[mode][d], want[mode][d])
                for key in ("R1", "R5", "R10", "MR"):
                    assert res[mode][d][key] == one[mode][d][key], (mode, d, key)


# ---- 6. the feature does what it claims --------------------------------------------------------------------------------------
def _hub_set(hub=5, n=N, scale=3.0):
    t, v, tm, vm = synth.make_samples(2024, "test", n, Nt, Nv)
    u = synth.normal(2024, "test/shared", (1, 1, t.shape[-1])).astype(np.float32) * scale
    t = (t + u).astype(np.float32)                           # the texts share a direction u: their mean direction
    v[hub] = u[0] + 0.5 * synth.normal(2024, "test/hub", (Nv, t.shape[-1])).astype(np.float32)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, v, tm.astype(np.float32), vm.astype(np.float32)))


def test_is_and_dsl_reduce_a_planted_hub():
    hub = 5
    m = _model()
    args = SimpleNamespace(world_size=1)
    # the weakest push toward the mean text direction that makes video `hub` THE hub: in more than half of the top-10 lists
    # and at the largest N_k (a hub in every list with a wide margin stays in DSL's lists: S * softmax keeps it above the
    # other columns' small weights)
    for scale in (0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0):
        t, v, tm, vm = _hub_set(hub, scale=scale)
        raw, _ = evaluator.sharded_metrics_with_hubness(m, t, v, tm, vm, args, 10)
        occ = raw["hubness"]["occurrence"]
        if occ[hub] == occ.max() and occ[hub] > N // 2:
            break
    assert occ[hub] == occ.max() and occ[hub] > N // 2, occ[hub]
    for mode in ("is", "dsl"):
        t2v, _ = evaluator.sharded_normalised_metrics(m, t, v, tm, vm, args, mode, BETA, hubness_k=10)
        h = t2v["hubness"]
        assert h["occurrence"][hub] < occ[hub], (mode, scale, h["occurrence"][hub], occ[hub])
        assert h["skewness"] < raw["hubness"]["skewness"], (mode, scale, h["skewness"], raw["hubness"]["skewness"])


def test_qbnorm_normalises_exactly_the_queries_whose_top1_is_the_active_video():
    hub = 5
    m = _model()
    t, v, tm, vm = _hub_set(hub)
    # every bank text points at the hub's direction: the top-1 of each bank text is the hub, so A_v = {hub} at qb_k = 1
    noise = torch.from_numpy(synth.normal(2024, "test/bank", (16, Nt, t.shape[-1])).astype(np.float32)).to(DEV)
    bt = (v[hub].mean(0)[None, None] + 0.05 * noise).contiguous()
    btm = torch.ones((16, Nt), device=DEV)
    bank = (bt, btm, v[:16].contiguous(), vm[:16].contiguous())
    args = SimpleNamespace(world_size=1)
    Qt, _ = evaluator._bank_slabs(m, t, v, tm, vm, bank, 1, 0)
    top = Qt.argmax(1).cpu().numpy()
    assert (top == hub).all(), top
    T, _ = evaluator.sharded_normalised_slabs(m, t, v, tm, vm, args, "qbnorm", BETA, querybank=bank, qb_k=1)
    S = _full(m, t, v, tm, vm, 1)
    T = T.cpu().numpy()
    changed = np.any(T != S, axis=1)
    assert np.array_equal(changed, S.argmax(1) == hub)
    assert changed.any()
    want = R.is_scores(S, BETA, ops.hubnorm_combine(ops.hubnorm_col_stats(Qt, BETA)[None]).cpu().numpy(), 0)
    assert _same_bits(T[changed], want[changed])
    _close(T[changed], R.is_scores(S, BETA, R.lse(Qt.cpu().numpy(), BETA, 0), 0)[changed].astype(np.float64), 1e-5)


# ---- 7. eval_epoch ------------------------------------------------------------------------------------------------------------
class Loader:
    def __init__(self, batches, dataset=None):
        self.batches, self.dataset = batches, dataset

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _batches(t, v, tm, vm, order, bs):
    return [(t[ix], tm[ix].long(), v[ix], vm[ix].long(), ix.clone(), ix.clone())
            for ix in (order[lo:lo + bs] for lo in range(0, len(order), bs))]


def _args(**over):
    return SimpleNamespace(world_size=1, rank=0, local_rank=0, logger=logging.getLogger("test_hubnorm"), **over)


def _strip(d):
    return {k: v for k, v in d.items() if k != "test_norm"}


def _bank_model(bank):
    m = _model()
    m.mb_ind = torch.arange(bank[0].shape[0], device=DEV)
    m.mb_feat_t, m.mb_mask_t, m.mb_feat_v, m.mb_mask_v = bank
    return m


def test_eval_epoch_single_sentence_with_each_mode(caplog):
    t, v, tm, vm = (x.cpu() for x in _testset())
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    loader = Loader(_batches(t, v, tm, vm, order, 32))
    bank = _bank()
    base = training.eval_epoch(_args(), _model(), loader, torch.device(DEV))
    assert training.eval_epoch(_args(test_norm="none"), _model(), loader, torch.device(DEV)) == base
    for mode in MODES:
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="test_hubnorm"):
            on = training.eval_epoch(_args(test_norm=mode, test_norm_beta=BETA, qb_k=1, hubness_k=5), _bank_model(bank), loader,
                                     torch.device(DEV))
        lines = [r.getMessage() for r in caplog.records]
        tag = evaluator.test_norm_label(mode, BETA)
        assert any(line.startswith(f"Text-to-Video {tag}: R@1") for line in lines), lines
        assert any(line.startswith(f"Video-to-Text {tag}: R@1") for line in lines)
        assert sum(f"{tag} Hubness@5" in line for line in lines) == 2
        strip = [{k: v for k, v in d.items() if k != "hubness"} for d in map(_strip, on)]
        assert strip[0] == base[0] and strip[1] == base[1]
        want = evaluator.sharded_normalised_metrics(_model(), t.to(DEV), v.to(DEV), tm.to(DEV), vm.to(DEV), _args(), mode, BETA,
                                                    querybank=bank, qb_k=1, hubness_k=5)
        _same_metrics(on[0]["test_norm"], want[0])
        _same_metrics(on[1]["test_norm"], want[1])
    with pytest.raises(ValueError, match="load_memory_bank"):
        training.eval_epoch(_args(test_norm="qbnorm"), _model(), loader, torch.device(DEV))


def test_eval_epoch_multi_sentence_with_dsl():
    Vn = 41
    sizes = 1 + (np.arange(Vn) * 3) % 4
    ends = np.cumsum(sizes)
    Ns = int(ends[-1])
    grp = np.searchsorted(ends, np.arange(Ns), side="right")
    t, _, tm, _ = (torch.from_numpy(a) for a in synth.make_samples(92, "test", Ns, Nt, Nv))
    _, v, _, vm = (torch.from_numpy(a) for a in synth.make_samples(93, "test", Vn, Nt, Nv))
    t = t + 0.4 * v[grp].mean(1, keepdim=True)
    dataset = SimpleNamespace(multi_sentence_per_video=True, cut_off_points=ends.tolist(), sentence_num=Ns, video_num=Vn)
    loader = Loader(_batches(t, v[grp], tm, vm[grp], torch.arange(Ns), 16), dataset)
    base = training.eval_epoch(_args(), _model(), loader, torch.device(DEV))
    on = training.eval_epoch(_args(test_norm="dsl"), _model(), loader, torch.device(DEV))
    assert _strip(on[0]) == base[0] and _strip(on[1]) == base[1]
    want = evaluator.sharded_normalised_metrics(_model(), t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float(), _args(),
                                                "dsl", BETA, cut_off_points=(ends - 1).tolist())
    _same_metrics(on[0]["test_norm"], want[0])
    _same_metrics(on[1]["test_norm"], want[1])


# ---- 8. main_retrieval.py ---------------------------------------------------------------------------------------------------
def test_main_retrieval_logs_normalised_metrics_only_with_the_flag():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--synthetic_test", "200"]
    outs = []
    for extra in ([], ["--test_norm", "dsl"], ["--test_norm", "qbnorm", "--hubness_k", "15"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()])
    plain, dsl, qb = outs
    assert not any("[DSL" in line or "[QB-Norm" in line for line in plain)
    extra_dsl = [line for line in dsl if "[DSL b=20]" in line]
    assert len(extra_dsl) == 1 and extra_dsl[0].startswith("text->video [DSL b=20] R@1")
    assert [line for line in dsl if "[DSL" not in line] == plain
    extra_qb = [line for line in qb if "[QB-Norm b=20]" in line]
    assert len(extra_qb) == 3 and sum("Hubness@15" in line for line in extra_qb) == 2
    raw_qb = [line for line in qb if "[QB-Norm" not in line and "Hubness@" not in line and "memory bank" not in line]
    assert raw_qb == plain
