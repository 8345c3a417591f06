"""GPU: local scaling -- CSLS, NICDM, LS (neighborretr_amd/csrc/nr_localscale.hip, evaluator.sharded_local_scaled_*).

The statistics kernel against the float32 restatement (localscale_ref) on the GPU's own lists of planted matrices (NaN lines,
infinities, signed zeros, short lines); the apply kernel bit for bit (csls) and to 2e-6 of the fp64 formulas (nicdm, ls) given
the GPU's own statistics; the same bits of T whatever the world size; the sharded evaluator under emulated ranks and two gloo
ranks, single- and multi-sentence, test-set and querybank neighbourhoods; that the three methods do take a planted hub out of
the lists; eval_epoch and main_retrieval.py with and without the flag.

"The same bits" below means: NaN in the same places (a NaN's sign and payload are not part of the definition) and the same
bits everywhere else."""
import functools
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hubness_ref as H
import hubnorm_ref as R
import localscale_ref as LS
from neighborretr_amd import comm, evaluator, modeling, ops, synth, training
from util import golden, params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
N, Nt, Nv = 96, 24, 12
MODES = LS.MODES
K = 10


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _close(got, want, rtol):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want, rtol=rtol, atol=rtol)


def _planted(n, L, seed):
    """Scores on a grid of 1/32 with signed zeros, infinities and NaN sprinkled in, an all-NaN row, a row of -inf only, an
    all-NaN column and a column of signed zeros only."""
    rng = np.random.default_rng(seed)
    S = (np.round(rng.standard_normal((n, L)) * 8) / 32).astype(np.float32)
    flat = S.reshape(-1)
    for val, frac in ((0.0, 0.05), (-0.0, 0.05), (np.inf, 0.005), (-np.inf, 0.02), (np.nan, 0.05)):
        at = rng.choice(flat.size, max(1, int(frac * flat.size)), replace=False)
        flat[at] = val
    if n > 2:
        S[0] = np.nan
        S[1, :] = -np.inf
    if L > 3:
        S[:, 2] = np.nan
        S[:, 3] = 0.0
        S[::2, 3] = -0.0
    return S


def _np(*xs):
    return tuple(x.cpu().numpy() for x in xs)


# ---- 1. statistics ------------------------------------------------------------------------------------------------------------
def _check_stats(idx, val, k):
    mean, kth = ops.localscale_stats(idx, val)
    n = idx.shape[0]
    assert mean.shape == (n,) and kth.shape == (n,) and mean.dtype == torch.float32 and kth.dtype == torch.float32
    i, v = _np(idx, val)
    present = (i >= 0).sum(1)
    want_mean, want_kth = LS.line_stats(i, v)
    mean_, kth_ = _np(mean, kth)
    assert np.array_equal(np.isnan(mean_), np.isnan(want_mean))
    assert np.isnan(mean_[present == 0]).all() and np.isnan(kth_[present == 0]).all()       # a list with no entry: both NaN
    inf_ = np.isinf(want_mean)
    assert np.array_equal(np.isinf(mean_), inf_) and np.array_equal(mean_[inf_], want_mean[inf_])      # and of the same sign
    fin = np.isfinite(want_mean)
    np.testing.assert_allclose(mean_[fin], want_mean[fin], rtol=1e-6, atol=0)
    assert _same_bits(kth_, want_kth)
    again = ops.localscale_stats(idx, val)                    # a second run gives the same bits
    assert _same_bits(again[0].cpu().numpy(), mean_) and _same_bits(again[1].cpu().numpy(), kth_)
    return present


# (n, k, L): L chosen so that the lists have short lines (fewer than k selectable entries) next to full ones
@pytest.mark.parametrize("n,k,L", [(1, 1, 1), (3, 5, 4), (130, 128, 129), (1000, 17, 37)])
def test_statistics_equal_the_restatement_on_the_gpus_own_lists(n, k, L):
    S = _planted(n, L, 7 * n + k)
    St = torch.from_numpy(S).to(DEV)
    present = _check_stats(*ops.slab_topk_rows(St, k), k)
    if n == 1:
        assert present[0] == 0                                # the one score is NaN: a list with no entry
    else:                                                     # the cases this test is about: short lines next to longer ones
        assert (present < k).any() and present.max() > present.min()
        # the column lists of the same matrix: column 2 has no entry at all
        present = _check_stats(*ops.slab_topk_cols(St, 0, k), k)
        assert present[2] == 0 and present.max() > 0


def test_statistics_refuse_what_is_not_a_pair_of_lists():
    idx = torch.zeros((4, 3), dtype=torch.int32, device=DEV)
    val = torch.zeros((4, 3), device=DEV)
    with pytest.raises(ValueError):
        ops.localscale_stats(idx, val[:, :2])
    with pytest.raises(ValueError):
        ops.localscale_stats(idx.long(), val)
    with pytest.raises(ValueError):
        ops.localscale_stats(torch.zeros((2, 129), dtype=torch.int32, device=DEV), torch.zeros((2, 129), device=DEV))
    m, k = ops.localscale_stats(idx[:0], val[:0])
    assert m.numel() == 0 and k.numel() == 0


# ---- 2. apply -----------------------------------------------------------------------------------------------------------------
def _gpu_stats(St, k):
    """((mean_row, kth_row), (mean_col, kth_col)) of one slab that is the whole matrix, from the GPU's own lists."""
    return ops.localscale_stats(*ops.slab_topk_rows(St, k)), ops.localscale_stats(*ops.slab_topk_cols(St, 0, k))


@pytest.mark.parametrize("n,L", [(1, 1), (3, 37), (130, 129), (90, 1000)])
def test_apply_csls_is_bit_exact_and_nicdm_and_ls_are_close(n, L):
    S = _planted(n, L, n + L)
    St = torch.from_numpy(S).to(DEV)
    rows, cols = _gpu_stats(St, 5)
    for mode in MODES:
        r, c = LS.pick(mode, rows), LS.pick(mode, cols)
        T = ops.localscale_apply(St, mode, r, c)
        got = T.cpu().numpy()
        want32 = LS.scores(S, mode, r.cpu().numpy(), c.cpu().numpy())
        assert np.array_equal(np.isnan(got), np.isnan(want32)), mode
        assert np.isnan(got[np.isnan(S)]).all()               # a NaN score stays NaN
        if mode == "csls":
            assert _same_bits(got, want32)
        else:
            want = LS.scores(S, mode, r.cpu().numpy(), c.cpu().numpy(), dtype=np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(want)), mode
            assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(got)], want[np.isinf(want)])
            ok = np.isfinite(want)
            np.testing.assert_allclose(got.astype(np.float64)[ok], want[ok], rtol=2e-6, atol=0)
        # a second run gives the same bits
        assert _same_bits(ops.localscale_apply(St, mode, r, c).cpu().numpy(), got)
        # a view misaligned by one float (the scalar path) gives the bits of the 16-byte path
        if L % 4 == 0 and n > 1:
            Sm = torch.empty(n * L + 1, device=DEV)[1:].view(n, L)
            Sm.copy_(St)
            assert Sm.data_ptr() % 16 == 4 and St.data_ptr() % 16 == 0
            assert _same_bits(ops.localscale_apply(Sm, mode, r, c).cpu().numpy(), got)


def test_apply_refuses_bad_arguments_and_takes_empty_slabs():
    St = torch.zeros((4, 8), device=DEV)
    r, c = torch.zeros((4,), device=DEV), torch.zeros((8,), device=DEV)
    with pytest.raises(ValueError):
        ops.localscale_apply(St, "is", r, c)
    with pytest.raises(ValueError):
        ops.localscale_apply(St, "csls", c, c)
    with pytest.raises(ValueError):
        ops.localscale_apply(St, "csls", r, r)
    assert ops.localscale_apply(St[:0], "ls", r[:0], c).shape == (0, 8)
    assert ops.localscale_apply(St[:, :0].contiguous(), "nicdm", r, c[:0]).shape == (4, 0)


# ---- 3. the same bits whatever the split --------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("bank", [False, True])
def test_the_scaled_matrix_has_the_same_bits_for_every_world_size(bank):
    n, L, M_t, M_v, k = 101, 67, 5, 11, 5                   # 5 bank texts: at W = 8 three ranks hold none of them
    S = _planted(n, L, 31)
    St = torch.from_numpy(S).to(DEV)
    Qt = _planted(M_t, L, 32)
    Qv = _planted(n, M_v, 33)
    Qt_t, Qv_t = torch.from_numpy(Qt).to(DEV), torch.from_numpy(Qv).to(DEV)
    first = {}
    for W in (1, 2, 3, 8):
        def fn(a, r, W=W):
            r0, r1 = evaluator.slab_bounds(n, W, r)
            q0, q1 = evaluator.slab_bounds(M_t, W, r)
            slabs = (Qt_t[q0:q1].contiguous(), Qv_t[r0:r1].contiguous()) if bank else None
            out = {}
            for mode in MODES:
                rs, cs = evaluator._local_scaling_stats(St[r0:r1].contiguous(), n, L, W, r, mode, k, slabs, M_t if bank else None)
                T = evaluator._local_scaled_from_slab(St[r0:r1].contiguous(), n, L, W, r, mode, k, slabs, M_t if bank else None)
                out[mode] = _np(T, rs, cs)
            return out
        outs = _emulated(W, fn)
        for mode in MODES:
            for o in outs:                                    # every rank's view of the column statistics
                assert _same_bits(o[mode][2], outs[0][mode][2]), (W, mode)
            whole = tuple(np.concatenate([o[mode][p] for o in outs]) for p in (0, 1)) + (outs[0][mode][2],)
            assert whole[0].shape == (n, L)
            if W == 1:
                first[mode] = whole
                # and they are the definition's: the statistics of the restatement's lists, csls's T bit for bit
                rows, cols = LS.neighbourhood_stats(S, k, Qt if bank else None, Qv if bank else None)
                if mode == "ls":
                    assert _same_bits(whole[1], rows[1]) and _same_bits(whole[2], cols[1])
                if mode == "csls":
                    assert _same_bits(whole[0], LS.scores(S, mode, whole[1], whole[2]))
            else:
                for p in range(3):
                    assert _same_bits(whole[p], first[mode][p]), (W, mode, p)


# ---- 4. the sharded evaluator ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model():
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _testset(n=N, seed=4242):
    t, v, tm, vm = synth.make_samples(seed, "test", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, v, tm.astype(np.float32), vm.astype(np.float32)))


@functools.lru_cache(maxsize=None)
def _bank(n=40, seed=77):
    t, v, tm, vm = synth.make_samples(seed, "train", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, tm.astype(np.float32), v, vm.astype(np.float32)))


def _full(m, a, b, am, bm, W):
    n = a.shape[0]
    return np.concatenate([evaluator._slab_similarity(m, a, b, am, bm, *evaluator.slab_bounds(n, W, r)).cpu().numpy()
                           for r in range(W)])


@functools.lru_cache(maxsize=None)
def _split_scores(W):
    """(S, Qt, Qv) of the test set and the bank as W slabs score them: computed once per W, shared, not written to."""
    m, (t, v, tm, vm), bank = _model(), _testset(), _bank()
    out = _full(m, t, v, tm, vm, W), _full(m, bank[0], v, bank[1], vm, W), _full(m, t, bank[2], tm, bank[3], W)
    for a in out:
        a.setflags(write=False)
    return out


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


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_evaluator_under_emulated_ranks_equals_the_restatement(mode, W, bank):
    m = _model()
    t, v, tm, vm = _testset()
    qb = _bank() if bank else None

    def fn(a, r):
        T = evaluator.sharded_local_scaled_slab(m, t, v, tm, vm, a, mode, k=K, bank=bank, querybank=qb)
        met = evaluator.sharded_local_scaled_metrics(m, t, v, tm, vm, a, mode, k=K, bank=bank, querybank=qb, hubness_k=5)
        return T.cpu().numpy(), met
    outs = _emulated(W, fn)
    T = np.concatenate([o[0] for o in outs])
    for _, met in outs:                                       # every rank returns the same dictionaries
        _same_metrics(met[0], outs[0][1][0])
        _same_metrics(met[1], outs[0][1][1])
    t2v, v2t = outs[0][1]
    for d in (t2v, v2t):
        assert d["mode"] == mode and d["k"] == K and d["bank"] is bank
    # the metrics are the rank rules and the lists of the GPU's own T
    assert t2v["cols"] == R.single_ranks(T).tolist() and v2t["cols"] == R.single_ranks(T.T).tolist()
    ht, hv = H.hubness(T, 5)
    assert np.array_equal(t2v["hubness"]["occurrence"], ht["occ"]) and np.array_equal(v2t["hubness"]["occurrence"], hv["occ"])
    # T against the definition, from the same split's S (and Qt, Qv)
    S, Qt, Qv = _split_scores(W)
    want = LS.local_scale(S, mode, K, Qt if bank else None, Qv if bank else None, dtype=np.float64)
    assert np.isfinite(want).all()
    _close(T, want, 1e-5)


def test_metrics_with_local_scaling_keep_the_raw_dictionaries():
    m = _model()
    t, v, tm, vm = _testset()
    a = SimpleNamespace(world_size=1)
    raw = evaluator.sharded_metrics_with_hubness(m, t, v, tm, vm, a, 5)
    both = evaluator.sharded_metrics_with_local_scaling(m, t, v, tm, vm, a, "nicdm", k=K, hubness_k=5)
    alone = evaluator.sharded_local_scaled_metrics(m, t, v, tm, vm, a, "nicdm", k=K, hubness_k=5)
    for d in range(2):
        _same_metrics({k_: v_ for k_, v_ in both[d].items() if k_ != "local_scaling"}, raw[d])
        _same_metrics(both[d]["local_scaling"], alone[d])
    with pytest.raises(ValueError):
        evaluator.sharded_local_scaled_metrics(m, t, v, tm, vm, a, "csls", k=0)
    with pytest.raises(ValueError):
        evaluator.sharded_local_scaled_metrics(m, t, v, tm, vm, a, "qbnorm")


# ---- 5. several sentences per video -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_multi_sentence_fixture_under_emulated_ranks(mode):
    g = golden("multi_sentence")
    S, cut = g["S"].astype(np.float32), g["cut_off_points"].tolist()
    Ns, V_ = S.shape
    ends = np.asarray(cut, dtype=np.int64) + 1
    St = torch.from_numpy(S).to(DEV)
    k = 3
    want = LS.local_scale(S, mode, k)
    for W in (1, 2, 3):
        def fn(a, r, W=W):
            r0, r1 = evaluator.slab_bounds(Ns, W, r)
            T = evaluator._local_scaled_from_slab(St[r0:r1].contiguous(), Ns, V_, W, r, mode, k)
            return T.cpu().numpy(), evaluator._metrics_from_normalised(T, T, Ns, V_, W, r, ends, 3)
        outs = _emulated(W, fn)
        T = np.concatenate([o[0] for o in outs])
        for o in outs:
            _same_metrics(o[1][0], outs[0][1][0])
            _same_metrics(o[1][1], outs[0][1][1])
        t2v, v2t = outs[0][1]
        want_t = training.RetrievalMetrics.multi_sentence_metrics_from_ranks(R.group_ranks(T, cut))
        want_v = training.RetrievalMetrics.metrics_from_ranks(R.single_ranks(R.group_max(T, cut)))
        for key in ("R1", "R5", "R10", "MedianR", "MeanR"):
            assert t2v[key] == want_t[key] and v2t[key] == want_v[key], (W, key)
        ht, hv = H.hubness(T, 3, cut)
        assert np.array_equal(t2v["hubness"]["occurrence"], ht["occ"]) and np.array_equal(v2t["hubness"]["occurrence"], hv["occ"])
        # a video's neighbourhood is its top-k sentences: the restatement's lists over the sentence rows
        _close(T, want.astype(np.float64), 1e-5)


# ---- 6. two gloo ranks, one child process each ----------------------------------------------------------------------------------
GLOO_CASES = (("csls", False), ("nicdm", True))


def _gloo_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    args = SimpleNamespace(world_size=world, local_rank=rank)
    m = _model()
    t, v, tm, vm = _testset()
    res = {mode: evaluator.sharded_local_scaled_metrics(m, t, v, tm, vm, args, mode, k=K, bank=bank, querybank=_bank(), hubness_k=5)
           for mode, bank in GLOO_CASES}
    torch.save(res, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_the_emulated_ranks_and_a_single_process(tmp_path):
    m = _model()
    t, v, tm, vm = _testset()
    world, port = 2, 29693
    out = str(tmp_path / "res")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--gloo-worker", str(r), str(world), str(port), out],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs, failed = [], False
    for p in procs:                                          # every child under its own time limit
        try:
            logs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            failed = True
            for q in procs:
                q.kill()
            logs.append(p.communicate()[0])
    assert not failed and all(p.returncode == 0 for p in procs), "\n".join(log[-2000:] for log in logs)
    for mode, bank in GLOO_CASES:
        def fn(a, r, mode=mode, bank=bank):
            return evaluator.sharded_local_scaled_metrics(m, t, v, tm, vm, a, mode, k=K, bank=bank, querybank=_bank(), hubness_k=5)
        want = _emulated(world, fn)[0]
        one = fn(SimpleNamespace(world_size=1), 0)
        for r in range(world):
            res = torch.load(f"{out}.{r}", weights_only=False)[mode]
            for d in range(2):
                _same_metrics(res[d], want[d])
                for key in ("R1", "R5", "R10", "MR"):
                    assert res[d][key] == one[d][key], (mode, d, key)


# ---- 7. the feature does what it claims -------------------------------------------------------------------------------------------
def _stated_matrix(seed=11, n=96, hub=5):
    """Scores on a grid of 1/256: noise, +0.25 for the true pairs, +0.3125 on one video's whole column (the hub)."""
    rng = np.random.default_rng(seed)
    S = np.round(rng.standard_normal((n, n)) * 32) / 256
    S[np.arange(n), np.arange(n)] += 0.25
    S[:, hub] += 0.3125
    return np.clip(S, -1, 1).astype(np.float32)


@pytest.mark.parametrize("mode", MODES)
def test_local_scaling_takes_a_planted_hub_out_of_the_lists(mode):
    hub, k, n = 5, 5, 96
    S = _stated_matrix()
    raw_occ = H.hubness(S, k)[0]["occ"]
    assert raw_occ[hub] == raw_occ.max() == 74               # the hub sits in 74 of the 96 top-5 lists
    Tr = LS.local_scale(S, mode, k)
    ref = H.hubness(Tr, k)
    assert 2 * ref[0]["occ"][hub] <= raw_occ[hub], (mode, ref[0]["occ"][hub])
    # recall under the project's own tie rule (one rank per entry equal to the own score) does not fall
    assert R.recall(R.single_ranks(Tr), 1) >= R.recall(R.single_ranks(S), 1)
    # the GPU's lists and ranks are the restatement's
    T = evaluator._local_scaled_from_slab(torch.from_numpy(S).to(DEV), n, n, 1, 0, mode, k)
    t2v, v2t = evaluator._metrics_from_normalised(T, T, n, n, 1, 0, None, k)
    assert np.array_equal(t2v["hubness"]["occurrence"], ref[0]["occ"]) and np.array_equal(v2t["hubness"]["occurrence"], ref[1]["occ"])
    assert t2v["cols"] == R.single_ranks(Tr).tolist() and v2t["cols"] == R.single_ranks(Tr.T).tolist()
    assert t2v["R1"] == R.recall(R.single_ranks(Tr), 1)


# ---- 8. eval_epoch and main_retrieval.py ----------------------------------------------------------------------------------------------
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
    return SimpleNamespace(world_size=1, rank=0, local_rank=0, logger=logging.getLogger("test_localscale"), **over)


def _fresh_model(bank=None):
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    m = m.to(DEV).eval()
    if bank is not None:
        m.mb_ind = torch.arange(bank[0].shape[0], device=DEV)
        m.mb_feat_t, m.mb_mask_t, m.mb_feat_v, m.mb_mask_v = bank
    return m


def test_eval_epoch_single_sentence_with_each_mode(caplog):
    t, v, tm, vm = (x.cpu() for x in _testset())
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    loader = Loader(_batches(t, v, tm, vm, order, 32))
    bank = _bank()
    dev = torch.device(DEV)
    base = training.eval_epoch(_args(), _fresh_model(), loader, dev)
    assert "local_scaling" not in base[0] and "local_scaling" not in base[1]
    assert training.eval_epoch(_args(local_scaling="none"), _fresh_model(), loader, dev) == base
    want_raw = evaluator.sharded_metrics(_model(), *_testset(), _args())
    assert base[0] == want_raw[0] and base[1] == want_raw[1]  # without the flag: what the evaluator gave before
    for mode, with_bank in (("csls", False), ("nicdm", True), ("ls", False)):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="test_localscale"):
            on = training.eval_epoch(_args(local_scaling=mode, local_scaling_k=K, local_scaling_bank=int(with_bank), hubness_k=5),
                                     _fresh_model(bank), loader, dev)
        lines = [r.getMessage() for r in caplog.records]
        tag = evaluator.local_scaling_label(mode, K, with_bank)
        assert any(line.startswith(f"Text-to-Video {tag}: R@1") for line in lines), lines
        assert any(line.startswith(f"Video-to-Text {tag}: R@1") for line in lines)
        assert sum(f"{tag} Hubness@5" in line for line in lines) == 2
        strip = [{k_: v_ for k_, v_ in d.items() if k_ not in ("local_scaling", "hubness")} for d in on]
        assert strip[0] == base[0] and strip[1] == base[1]
        want = evaluator.sharded_local_scaled_metrics(_model(), *_testset(), _args(), mode, k=K, bank=with_bank, querybank=bank,
                                                      hubness_k=5)
        _same_metrics(on[0]["local_scaling"], want[0])
        _same_metrics(on[1]["local_scaling"], want[1])
    with pytest.raises(ValueError, match="load_memory_bank"):
        training.eval_epoch(_args(local_scaling="csls", local_scaling_bank=1), _fresh_model(), loader, dev)
    with pytest.raises(ValueError, match="local_scaling"):
        training.eval_epoch(_args(local_scaling="csls", test_norm="is"), _fresh_model(), loader, dev)


def test_eval_epoch_multi_sentence_with_csls():
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
    dev = torch.device(DEV)
    base = training.eval_epoch(_args(), _fresh_model(), loader, dev)
    on = training.eval_epoch(_args(local_scaling="csls", local_scaling_k=4), _fresh_model(), loader, dev)
    for d in range(2):
        assert {k_: v_ for k_, v_ in on[d].items() if k_ != "local_scaling"} == base[d]
    want = evaluator.sharded_local_scaled_metrics(_model(), t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float(), _args(),
                                                  "csls", k=4, cut_off_points=(ends - 1).tolist())
    _same_metrics(on[0]["local_scaling"], want[0])
    _same_metrics(on[1]["local_scaling"], want[1])


def test_main_retrieval_logs_local_scaling_only_with_the_flag():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--synthetic_test", "200"]
    outs = []
    for extra in ([], ["--local_scaling", "csls"],
                  ["--local_scaling", "nicdm", "--local_scaling_bank", "1", "--local_scaling_k", "7", "--hubness_k", "15"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()])
    plain, csls, qb = outs
    assert not any("CSLS" in line or "NICDM" in line or "local_scaling" in line for line in plain)
    extra_csls = [line for line in csls if "[CSLS k=10]" in line]
    assert len(extra_csls) == 1 and extra_csls[0].startswith("text->video [CSLS k=10] R@1")
    assert "video->text [CSLS k=10] R@1" in extra_csls[0]
    assert [line for line in csls if "[CSLS" not in line] == plain
    extra_qb = [line for line in qb if "[QB-NICDM k=7]" in line]
    assert len(extra_qb) == 3 and sum("Hubness@15" in line for line in extra_qb) == 2
    raw_qb = [line for line in qb if "[QB-NICDM" not in line and "Hubness@" not in line and "memory bank" not in line]
    assert raw_qb == plain


if __name__ == "__main__":                                   # one gloo rank of the two-rank test
    if len(sys.argv) == 6 and sys.argv[1] == "--gloo-worker":
        _gloo_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
