"""GPU: top-k selection and hubness (neighborretr_amd/csrc/nr_topk.hip, evaluator.sharded_topk / sharded_hubness).

The kernels against the reference's neighbour sets (c2_b128's nb_mask, c3 / c4's nb_idx) and, bit for bit, against the NumPy
restatement of the definitions (hubness_ref): every k, awkward shapes, planted ties, signed zeros, infinities, NaN lines.
Column lists of row slabs merged over W slabs equal the whole matrix's.  The sharded evaluator under emulated ranks and two
gloo ranks equals the single-process result; the multi-sentence fixture in both directions; eval_epoch with and without
hubness."""
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hubness_ref as H
from neighborretr_amd import comm, evaluator, modeling, ops, synth, training
from neighborretr_amd.metrics import RetrievalMetrics
from util import golden, params, problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
N, Nt, Nv = 203, 24, 12


def _rows(S, k):
    i, v = ops.slab_topk_rows(torch.as_tensor(S).to(DEV), k)
    return i.cpu().numpy(), v.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _check_lists(S, k):
    ri, rv = _rows(S, k)
    ei, ev = H.topk_lists(S, k)
    assert np.array_equal(ri, ei), (S.shape, k)
    assert _same_bits(rv, ev), (S.shape, k)
    ci, cv = ops.slab_topk_cols(torch.from_numpy(S).to(DEV), 0, k)
    ei, ev = H.topk_lists(S.T.copy(), k)
    assert np.array_equal(ci.cpu().numpy(), ei), (S.shape, k)
    assert _same_bits(cv.cpu().numpy(), ev), (S.shape, k)


# ---- 1. the reference's neighbour sets ------------------------------------------------------------------------------------
def test_c2_b128_rows_and_column_occurrences_match_reference_nb_mask():
    g = golden("c2_b128")
    K = int(g["K"])
    S = g["S"].copy()
    np.fill_diagonal(S, np.nan)                               # the diagonal is never a neighbour: NaN is never selected
    idx, _ = _rows(S, K)
    mask = np.zeros_like(g["nb_mask"])
    np.put_along_axis(mask, idx.astype(np.int64), 1, axis=1)
    assert np.array_equal(mask, g["nb_mask"])
    occ, good = ops.topk_occurrences(torch.from_numpy(idx).to(DEV), S.shape[1], torch.arange(128, dtype=torch.int32, device=DEV),
                                     torch.arange(1, 129, dtype=torch.int32, device=DEV))
    assert np.array_equal(occ.cpu().numpy(), g["nb_mask"].sum(0))
    assert int(good.sum()) == 0                               # the diagonal (each row's own item) was excluded


@pytest.mark.parametrize("name", ["c3_b1024", "c4_b128_full"])
def test_large_fixture_neighbour_sets(name):
    g = golden(name)
    B, Nt_, Nv_, M, K = (int(g[k]) for k in ("B", "Nt", "Nv", "M", "K"))
    x = problem(int(g["seed"]), B, Nt_, Nv_, M, device=DEV)
    m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K), precision="bf16x3")
    m.load_state_dict(params(), strict=False)
    m = m.to(DEV).train()                                      # as test_fixtures_large_gpu builds it
    with torch.no_grad():
        m.clip.logit_scale.fill_(float(np.log(100.0)))
        S, _ = m.get_similarity_logits(x["text_feat"], x["video_feat"], x["text_mask"], x["video_mask"])
        S = S.detach().clone()
        S.fill_diagonal_(float("nan"))
    idx, _ = ops.slab_topk_rows(S.contiguous(), K)
    assert np.array_equal(np.sort(idx.cpu().numpy(), axis=1), g["nb_idx"].astype(np.int32))


# ---- 2. the kernels against the definitions ------------------------------------------------------------------------------
def _planted(n, L, seed):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, L)).astype(np.float32)
    S = np.round(S * 4) / 4                                   # many exact ties
    flat = S.reshape(-1)
    for val, frac in ((0.0, 0.05), (-0.0, 0.05), (np.inf, 0.01), (-np.inf, 0.02), (np.nan, 0.05)):
        at = rng.choice(flat.size, max(1, int(frac * flat.size)), replace=False)
        flat[at] = val
    S[0] = np.nan                                             # a line that is entirely NaN
    if n > 2:
        S[1, :] = 0.0
        S[1, ::2] = -0.0                                      # a line of signed zeros only
    if L > 2:
        S[:, 2] = np.nan                                      # a column that is entirely NaN
    return S


@pytest.mark.parametrize("k", [1, 5, 15, 64, 128])
@pytest.mark.parametrize("n,L", [(7, 203), (90, 1000), (3, 37), (130, 129), (5, 1)])
def test_kernel_sweep_equals_reference_bit_for_bit(k, n, L):
    _check_lists(_planted(n, L, 1000 * k + n), k)


def test_long_lines_read_from_memory_equal_reference():
    # lines longer than the LDS key cache take the uncached form of the kernel
    rng = np.random.default_rng(4)
    S = (np.round(rng.standard_normal((3, 20000)) * 8) / 8).astype(np.float32)
    S[1, 5::7] = np.nan
    for k in (1, 17, 128):
        _check_lists(S, k)


def test_lists_are_reproducible_run_to_run():
    S = torch.from_numpy(_planted(64, 777, 9)).to(DEV)
    a = ops.slab_topk_cols(S, 3, 15)
    b = ops.slab_topk_cols(S, 3, 15)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- 3. column lists of slabs, merged -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("k", [1, 15, 128])
def test_column_lists_of_slabs_merge_to_the_whole_matrix(W, k):
    S = _planted(101, 67, 77 + W)
    St = torch.from_numpy(S).to(DEV)
    parts_i, parts_v = [], []
    for r in range(W):
        r0, r1 = evaluator.slab_bounds(S.shape[0], W, r)
        i, v = ops.slab_topk_cols(St[r0:r1].contiguous(), r0, k)
        parts_i.append(i)
        parts_v.append(v)
    mi, mv = ops.topk_merge(torch.stack(parts_i), torch.stack(parts_v))
    ei, ev = H.topk_lists(S.T.copy(), k)
    assert np.array_equal(mi.cpu().numpy(), ei)
    assert _same_bits(mv.cpu().numpy(), ev)


def test_merge_of_a_gallery_scored_in_chunks():
    S = _planted(40, 300, 5)
    St = torch.from_numpy(S).to(DEV)
    k, cuts = 20, [0, 64, 65, 200, 300]
    parts = [ops.slab_topk_rows(St[:, a:b].contiguous(), k) for a, b in zip(cuts[:-1], cuts[1:])]
    idx = torch.stack([torch.where(p[0] >= 0, p[0] + a, p[0]) for p, a in zip(parts, cuts[:-1])])     # chunk -> gallery index
    mi, mv = ops.topk_merge(idx.contiguous(), torch.stack([p[1] for p in parts]))
    ei, ev = H.topk_lists(S, k)
    assert np.array_equal(mi.cpu().numpy(), ei) and _same_bits(mv.cpu().numpy(), ev)


# ---- 4. the sharded evaluator ----------------------------------------------------------------------------------------------
def _model():
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    return m.to(DEV).eval()


def _testset():
    t, v, tm, vm = synth.make_samples(4242, "test", N, Nt, Nv)
    v[17] = v[16]                                             # two identical videos: exact ties in both directions
    vm[17] = vm[16]
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, v, tm, vm))


def _full_similarity(m, t, v, tm, vm, W=1):
    """The matrix W ranks score, slab by slab with the call each rank makes.  The split-bf16 similarity of a row can differ in
    its last bit with the row split (observed: 1 ulp between W = 1 and W = 2), so scores are pinned per split; the selected
    indices and the occurrence counts are pinned across splits."""
    n = t.shape[0]
    return np.concatenate([evaluator._slab_similarity(m, t, v, tm.float(), vm.float(), *evaluator.slab_bounds(n, W, r)).cpu().numpy()
                           for r in range(W)])


def _emulated(W, fn):
    world = comm.EmulatedWorld(W, real_collectives=False)
    out = {}

    def run(r):
        c = world.comm(r)
        with comm.use(c):
            c.begin_step()
            out[r] = fn(SimpleNamespace(world_size=W))
    world.settle(run)
    return [out[r] for r in range(W)]


def _same_hub(a, b):
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        else:
            assert a[key] == b[key], key


def _against_ref(hub, ref, k, n_queries):
    assert np.array_equal(hub["occurrence"], ref["occ"]) and np.array_equal(hub["good_occurrence"], ref["good"])
    mine = RetrievalMetrics.hubness_from_occurrences(ref["occ"], ref["good"], k, n_queries)
    _same_hub(hub, mine)
    for key, want in ref["summary"].items():
        assert hub[key] == pytest.approx(want, rel=1e-12, abs=1e-12), key


@pytest.mark.parametrize("k", [1, 15])
def test_sharded_topk_and_hubness_under_emulated_ranks(k):
    m = _model()
    t, v, tm, vm = _testset()
    first = None
    for W in (1, 2, 3, 4):
        rt, rv = H.hubness(_full_similarity(m, t, v, tm, vm, W), k)
        tops = _emulated(W, lambda a: evaluator.sharded_topk(m, t, v, tm.float(), vm.float(), k, a))
        hubs = _emulated(W, lambda a: evaluator.sharded_hubness(m, t, v, tm.float(), vm.float(), a, k=k))
        for r in range(W):
            ti, tv, vi, vv = (x.cpu().numpy() for x in tops[r])
            assert np.array_equal(ti, rt["idx"]) and _same_bits(tv, rt["val"]), (W, r)
            assert np.array_equal(vi, rv["idx"]) and _same_bits(vv, rv["val"]), (W, r)
            _against_ref(hubs[r][0], rt, k, N)
            _against_ref(hubs[r][1], rv, k, N)
            if first is None:
                first = (ti, vi, hubs[r])
            assert np.array_equal(ti, first[0]) and np.array_equal(vi, first[1]), W
            _same_hub(hubs[r][0], first[2][0])
            _same_hub(hubs[r][1], first[2][1])


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from neighborretr_amd.evaluator import sharded_hubness, sharded_topk
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    args = SimpleNamespace(world_size=world, local_rank=rank)
    m = _model()
    t, v, tm, vm = _testset()
    tops = [x.cpu() for x in sharded_topk(m, t, v, tm.float(), vm.float(), 15, args)]
    hubs = sharded_hubness(m, t, v, tm.float(), vm.float(), args, k=15)
    torch.save({"tops": tops, "hubs": hubs}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_hubness_two_gloo_ranks_equal_single_process(tmp_path):
    import torch.multiprocessing as mp
    m = _model()
    t, v, tm, vm = _testset()
    world, port = 2, 29653
    rt, rv = H.hubness(_full_similarity(m, t, v, tm, vm, world), 15)
    r1t, r1v = H.hubness(_full_similarity(m, t, v, tm, vm), 15)
    assert np.array_equal(rt["idx"], r1t["idx"]) and np.array_equal(rv["idx"], r1v["idx"])        # the same lists as one process
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        res = torch.load(f"{out}.{r}", weights_only=False)
        ti, tv, vi, vv = (x.numpy() for x in res["tops"])
        assert np.array_equal(ti, rt["idx"]) and _same_bits(tv, rt["val"])
        assert np.array_equal(vi, rv["idx"]) and _same_bits(vv, rv["val"])
        _against_ref(res["hubs"][0], rt, 15, N)
        _against_ref(res["hubs"][1], rv, 15, N)


# ---- 5. multi-sentence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 15])
def test_multi_sentence_fixture_both_directions(k):
    g = golden("multi_sentence")
    S, cut = g["S"], g["cut_off_points"].tolist()
    assert int(np.isnan(S).sum()) == 2
    Ns, V = S.shape
    rt, rv = H.hubness(S, k, cut)
    ends = np.asarray(cut, dtype=np.int64) + 1
    St = torch.from_numpy(S).to(DEV)
    for W in (1, 2, 3):
        def fn(a, W=W):
            r = comm.get_rank() if W > 1 else 0
            r0, r1 = evaluator.slab_bounds(Ns, W, r)
            slab = St[r0:r1].contiguous()
            return (evaluator._topk_from_slab(slab, Ns, V, k, W, r), evaluator._hubness_from_slab(slab, Ns, V, k, W, r, ends))
        for (ti, tv, vi, vv), (ht, hv) in _emulated(W, fn):
            assert np.array_equal(ti.cpu().numpy(), rt["idx"]) and _same_bits(tv.cpu().numpy(), rt["val"]), W
            assert np.array_equal(vi.cpu().numpy(), rv["idx"]) and _same_bits(vv.cpu().numpy(), rv["val"]), W
            _against_ref(ht, rt, k, Ns)
            _against_ref(hv, rv, k, V)


# ---- 6. the callers -------------------------------------------------------------------------------------------------------
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
    return SimpleNamespace(world_size=1, rank=0, local_rank=0, logger=logging.getLogger("test_hubness"), **over)


def _strip(m):
    return {k: v for k, v in m.items() if k != "hubness"}


def test_eval_epoch_single_sentence_with_and_without_hubness(caplog):
    t, v, tm, vm = (x.cpu() for x in _testset())
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    loader = Loader(_batches(t, v, tm, vm, order, 32))
    with caplog.at_level(logging.INFO, logger="test_hubness"):
        base = training.eval_epoch(_args(), _model(), loader, torch.device(DEV))
        off = training.eval_epoch(_args(hubness_k=0), _model(), loader, torch.device(DEV))
        assert not any("Hubness" in r.getMessage() for r in caplog.records)
        caplog.clear()
        on = training.eval_epoch(_args(hubness_k=15), _model(), loader, torch.device(DEV))
        lines = [r.getMessage() for r in caplog.records if "Hubness@15" in r.getMessage()]
    assert off == base and "hubness" not in off[0] and "hubness" not in off[1]
    assert _strip(on[0]) == base[0] and _strip(on[1]) == base[1]
    assert len(lines) == 2 and lines[0].startswith("Text-to-Video") and lines[1].startswith("Video-to-Text")
    m = _model()
    ht, hv = evaluator.sharded_hubness(m, t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float(), _args(), k=15)
    _same_hub(on[0]["hubness"], ht)
    _same_hub(on[1]["hubness"], hv)


def test_eval_epoch_multi_sentence_with_hubness():
    V = 41
    sizes = 1 + (np.arange(V) * 3) % 4
    ends = np.cumsum(sizes)
    Ns = int(ends[-1])
    grp = np.searchsorted(ends, np.arange(Ns), side="right")
    t, _, tm, _ = (torch.from_numpy(a) for a in synth.make_samples(92, "test", Ns, Nt, Nv))
    _, v, _, vm = (torch.from_numpy(a) for a in synth.make_samples(93, "test", V, Nt, Nv))
    t = t + 0.4 * v[grp].mean(1, keepdim=True)
    dataset = SimpleNamespace(multi_sentence_per_video=True, cut_off_points=ends.tolist(), sentence_num=Ns, video_num=V)
    loader = Loader(_batches(t, v[grp], tm, vm[grp], torch.arange(Ns), 16), dataset)
    base = training.eval_epoch(_args(), _model(), loader, torch.device(DEV))
    on = training.eval_epoch(_args(hubness_k=15), _model(), loader, torch.device(DEV))
    assert _strip(on[0]) == base[0] and _strip(on[1]) == base[1]
    S = _full_similarity(_model(), t.to(DEV), v.to(DEV), tm.to(DEV), vm.to(DEV))
    rt, rv = H.hubness(S, 15, (ends - 1).tolist())
    _against_ref(on[0]["hubness"], rt, 15, Ns)
    _against_ref(on[1]["hubness"], rv, 15, V)


def test_main_retrieval_logs_hubness_only_with_the_flag():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--synthetic_test", "200"]
    outs = []
    for extra in ([], ["--hubness_k", "15"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()])
    plain, hub = outs
    assert not any("Hubness@" in line for line in plain)
    assert sum("Hubness@15" in line for line in hub) == 2
    assert [line for line in hub if "Hubness@" not in line] == plain
