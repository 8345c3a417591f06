"""GPU: two-stage retrieval.  nr_local_level_cand against fp64 on every tile form, with padding, out-of-range
entries, duplicates and masked items in the lists; the pooled prefilter against fp64; the pipeline's logic against the restatement
of tests/rerank_ref.py, fed the GPU's own lists; C = N against the exhaustive truth; two gloo ranks; the exhaustive mode; the
command line."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rerank_ref as R
from neighborretr_amd import evaluator, hip, modeling, ops, search, synth
from util import maxdiff, params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
N, Nt, Nv = 203, 24, 12             # not a multiple of the rank count or of any tile size
ARGS = SimpleNamespace(world_size=1)


def _model():
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    return m.to(DEV).eval()


def _samples(seed, n, nt=Nt, nv=Nv):
    return tuple(torch.from_numpy(a) for a in synth.make_samples(seed, "test", n, nt, nv))


# ---- 1. the kernel against fp64 ---------------------------------------------------------------------------------------------------------
SHAPES = [
    # n_q, Nq, n_g, Ng, C, d
    (5, 24, 37, 12, 7, 512),       # MI = 1: the 32-row query tile; 8 candidates per run, a ragged last run
    (3, 64, 21, 64, 3, 512),       # 2 candidates per 128 columns, two runs
    (9, 20, 11, 7, 11, 512),       # token counts that do not divide the tile; C = n_g
    (4, 77, 3, 100, 2, 512),       # one candidate per run, 96-row query tile
    (2, 3, 7, 6, 1, 512),          # C = 1
    (6, 24, 300, 12, 128, 512),    # the longest list: 16 runs per query
    (5, 24, 9, 12, 4, 128),        # d = 128: two K slices
    # the tile forms (MI, NI) the shapes above leave out: (2, 3), (3, 3), (4, 3), (4, 4)
    (3, 40, 10, 12, 5, 512),
    (3, 70, 6, 24, 3, 512),
    (3, 128, 5, 48, 3, 512),       # the most query tokens the kernel takes
    (3, 100, 4, 128, 2, 512),      # the most gallery tokens: one candidate per 128-column run
]
_REF = {}


def _kernel_case(n_q, Nq, n_g, Ng, C, d):
    """Inputs as in test_local_level_matches_oracle (a fully masked gallery item, random softmax weights) plus a fully masked query
    and a repeated query; the fp64 matrix; candidate lists with padding, out-of-range entries and duplicates.  Built once."""
    key = (n_q, Nq, n_g, Ng, C, d)
    if key in _REF:
        return _REF[key]
    g = torch.Generator().manual_seed(n_q * 1000 + n_g)
    base = torch.randn(max(n_q, n_g), 1, d, generator=g)
    q = base[:n_q] + 4 * torch.randn(n_q, Nq, d, generator=g)
    v = base[:n_g] + 4 * torch.randn(n_g, Ng, d, generator=g)
    qm = (torch.arange(Nq)[None] < torch.randint(1, Nq + 1, (n_q, 1), generator=g)).long()
    vm = (torch.arange(Ng)[None] < torch.randint(1, Ng + 1, (n_g, 1), generator=g)).long()
    w_q = torch.softmax(torch.randn(n_q, Nq, generator=g), -1)
    w_g = torch.softmax(torch.randn(n_g, Ng, generator=g), -1)
    if n_g > 2:
        vm[2] = 0                                   # a fully masked gallery item
    qm[1] = 0                                       # a fully masked query
    if n_q > 2:                                     # the last query repeats query 0: the same pairs in two queries' lists
        q[n_q - 1], qm[n_q - 1], w_q[n_q - 1] = q[0], qm[0], w_q[0]
    S = R.similarity(q, qm, w_q, v, vm, w_g).numpy()
    cand = torch.randint(0, n_g, (n_q, C), generator=g).int()
    for i, bad in enumerate((-1, n_g, -5, 2 ** 30, -1)):            # padding, an index >= n_g, an index < -1
        cand[(i + 1) % n_q, (2 * i + 1) % C] = bad
    cand[0, 0] = min(2, n_g - 1)                    # the masked item, ...
    if C > 1:
        cand[0, C - 1] = cand[0, 0]                 # ... twice in one list, ...
        cand[n_q - 1, C // 2] = cand[0, 0]          # ... and in the list of the repeated query at another position
    _REF[key] = (q, qm, w_q, v, vm, w_g, S, cand)
    return _REF[key]


def _prepared(x, mask):
    """Prepared tokens of x [n, tokens, d].  nr_prepare_tokens takes widths that are multiples of 256; another width (the d = 128
    case) is normalised and masked with torch and split by nr_split_bf16: the same hi/lo images by another route."""
    x, mask = x.to(DEV), mask.to(DEV)
    d = x.shape[-1]
    if d % 256 == 0:
        return ops.prepare_tokens(x, mask)
    xn = (torch.nn.functional.normalize(x, dim=-1) * mask[..., None]).reshape(-1, d)
    hi, lo = ops.split_bf16(xn)
    return ops.Prepared(hi, lo, None, None, xn.shape[0], d)


def _check_lists(out, S, cand, tol, swapped=False):
    out, cand = out.cpu().numpy(), cand.cpu().numpy()
    n_g = S.shape[0] if swapped else S.shape[1]
    ok = (cand >= 0) & (cand < n_g)
    assert np.all(np.isneginf(out[~ok])) and np.all(np.isfinite(out[ok]))
    want = R.pair_scores(S.T if swapped else S, cand)
    worst = float(np.abs(out[ok] - want[ok]).max())
    print(f"max |out - fp64| = {worst:.3e} (bound {tol:g})")
    assert worst < tol


@pytest.mark.parametrize("n_q,Nq,n_g,Ng,C,d", SHAPES)
@pytest.mark.parametrize("prec,tol", [(hip.PREC_BF16X3, 2e-6), (hip.PREC_BF16, 1e-3)])
def test_candidate_scores_match_fp64(n_q, Nq, n_g, Ng, C, d, prec, tol):
    q, qm, w_q, v, vm, w_g, S, cand = _kernel_case(n_q, Nq, n_g, Ng, C, d)
    pq, pg = _prepared(q, qm), _prepared(v, vm)
    wq, wg, cd = w_q.to(DEV), w_g.to(DEV), cand.to(DEV)
    out = ops.local_level_cand(pq, pg, wq, wg, n_q, Nq, n_g, Ng, cd, prec)
    _check_lists(out, S, cand, tol)
    o, c = out.cpu(), cand
    bits = o.view(torch.int32)
    valid = (c >= 0) & (c < n_g)
    assert bool(valid[0, 0]) and float(o[1][valid[1]].abs().max() if valid[1].any() else 0.0) == 0.0      # the masked query: exact zeros
    if n_g > 2:
        assert float(o[c == 2].abs().max()) == 0.0                                                         # the masked item
    # identical pairs give identical bits: inside a list, and between the lists of query 0 and its repeat
    alias = {n_q - 1: 0} if n_q > 2 else {}
    seen = {}
    for i in range(n_q):
        for j in range(C):
            if valid[i, j]:
                first = seen.setdefault((alias.get(i, i), int(c[i, j])), int(bits[i, j]))
                assert first == int(bits[i, j]), (i, j)
    if C > 1:
        assert bits[0, 0] == bits[0, C - 1]
        if n_q > 2:
            assert bits[n_q - 1, C // 2] == bits[0, 0]
    # a list cut to its first half gives the same bits for that half: a pair's score does not depend on C
    h = max(1, C // 2)
    half = ops.local_level_cand(pq, pg, wq, wg, n_q, Nq, n_g, Ng, cd[:, :h].contiguous(), prec)
    assert torch.equal(half.cpu().view(torch.int32), bits[:, :h])
    # roles swapped: the gallery items as queries, the queries as the gallery (the formula is symmetric)
    g = torch.Generator().manual_seed(C)
    C2 = min(C, 5)
    cand2 = torch.randint(0, n_q, (n_g, C2), generator=g).int()
    cand2[0, 0] = -1
    out2 = ops.local_level_cand(pg, pq, wg, wq, n_g, Ng, n_q, Nq, cand2.to(DEV), prec)
    _check_lists(out2, S, cand2, tol, swapped=True)


def test_wrapper_refuses_lists_that_do_not_fit():
    q, qm, w_q, v, vm, w_g, _, cand = _kernel_case(*SHAPES[0])
    pq, pg = ops.prepare_tokens(q.to(DEV), qm.to(DEV)), ops.prepare_tokens(v.to(DEV), vm.to(DEV))
    with pytest.raises(ValueError, match="cand must be"):
        ops.local_level_cand(pq, pg, w_q.to(DEV), w_g.to(DEV), 5, 24, 37, 12, cand[:3].to(DEV))
    with pytest.raises(hip.NrHipError):
        ops.local_level_cand(pq, pg, w_q.to(DEV), w_g.to(DEV), 5, 24, 37, 12, cand.long().to(DEV))
    with pytest.raises(hip.NrHipError, match="nr_local_level_cand failed"):
        ops.local_level_cand(pq, pg, w_q.to(DEV), w_g.to(DEV), 5, 24, 37, 12, torch.zeros((5, 129), dtype=torch.int32, device=DEV))


# ---- 2. the prefilter ---------------------------------------------------------------------------------------------------------------------
def test_prefilter_matches_fp64_and_does_not_depend_on_the_chunk():
    C = 16
    t, v, tm, vm = _samples(4242, N)
    m = _model()
    index = search.GalleryIndex(m, v.to(DEV), vm.to(DEV).float())
    with torch.no_grad():
        qs = search._Side(m, t.to(DEV), tm.to(DEV).float(), "text")
        got = index.coarse_scores(qs.pooled).cpu().numpy()
    want = R.coarse(R.pooled(t, tm, qs.w.cpu()), R.pooled(v, vm, index.items.w.cpu()))
    worst = float(np.abs(got - want).max())
    print(f"max |coarse - fp64| = {worst:.3e} (bound 2e-6)")
    assert worst < 2e-6
    cand, fine = index.candidates(t.to(DEV), tm.to(DEV).float(), C, chunk=256)
    cand7, fine7 = index.candidates(t.to(DEV), tm.to(DEV).float(), C, chunk=7)
    assert torch.equal(cand, cand7) and torch.equal(fine.view(torch.int32), fine7.view(torch.int32))
    cand = cand.cpu().numpy()
    assert np.all(np.diff(cand, axis=1) > 0) and cand.min() >= 0 and cand.max() < N          # ascending, no padding, no repeats
    for i in range(N):
        kth = np.sort(want[i])[-C]
        assert np.all(want[i, cand[i]] >= kth - 4e-6), i
        assert set(np.nonzero(want[i] > kth + 4e-6)[0]) <= set(cand[i].tolist()), i


# ---- 3. the pipeline's logic, exact, on the GPU's own lists ----------------------------------------------------------------------------------
def _lists(m, gallery, gmask, side, queries, qmask, C):
    cand, fine = search.GalleryIndex(m, gallery.to(DEV), gmask.to(DEV).float(), side).candidates(queries.to(DEV), qmask.to(DEV).float(), C)
    return cand.cpu().numpy(), fine.cpu().numpy()


def test_search_and_evaluation_equal_the_restatement_on_the_same_lists():
    C, k = 8, 5
    t, v, tm, vm = _samples(4242, N)
    m = _model()
    index = search.GalleryIndex(m, v.to(DEV), vm.to(DEV).float())
    idx, val, cand, fine = index.search(t.to(DEV), tm.to(DEV).float(), k, C, return_candidates=True)
    want_idx, want_val = R.final_order(cand.cpu().numpy(), fine.cpu().numpy(), k)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(val.cpu().numpy(), want_val)
    idx2, val2 = index.search(t.to(DEV), tm.to(DEV).float(), k, C)
    assert torch.equal(idx, idx2) and torch.equal(val, val2)
    with pytest.raises(ValueError, match="1 <= k <= n_candidates"):
        index.search(t.to(DEV), tm.to(DEV).float(), 9, C)
    cand_t, fine_t = cand.cpu().numpy(), fine.cpu().numpy()
    cand_v, fine_v = _lists(m, t, tm, "text", v, vm, C)
    got = evaluator.two_stage_evaluation(m, t.to(DEV), v.to(DEV), tm.to(DEV), vm.to(DEV), ARGS, C)
    want = R.single_sentence(cand_t, fine_t, cand_v, fine_v, C)
    assert got[0] == want[0] and got[1] == want[1]
    assert got[0]["R10"] is None and got[0]["R5"] is not None and 0 < got[0]["cand_recall"] <= 100


def test_multi_sentence_evaluation_equals_the_restatement_on_the_same_lists():
    C = 8
    sizes = [3, 1, 4, 2, 5, 1, 3, 2, 6, 1, 4, 3]                    # ragged groups, one-sentence groups included
    ends = np.cumsum(sizes)
    Ns, V = int(ends[-1]), len(sizes)
    t, v, tm, vm = _samples(99, Ns)
    group = np.searchsorted(ends, np.arange(Ns), side="right")
    first = np.concatenate(([0], ends[:-1]))
    v, vm = v[first], vm[first]                                      # video g belongs to the sentences of group g
    t = t + 0                                                        # sentences of one group: noisy copies of the group's first
    t = t[first[group]] + 0.5 * (t - t[first[group]])
    tm = tm[first[group]]
    m = _model()
    cand_t, fine_t = _lists(m, v, vm, "video", t, tm, C)
    cand_v, fine_v = _lists(m, t, tm, "text", v, vm, C)
    got = evaluator.two_stage_evaluation(m, t.to(DEV), v.to(DEV), tm.to(DEV), vm.to(DEV), ARGS, C, cut_off_points=(ends - 1).tolist())
    want = R.multi_sentence(cand_t, fine_t, cand_v, fine_v, ends, C)
    assert got[0] == want[0] and got[1] == want[1]
    assert got[0]["cand_recall"] > 0 and got[1]["cand_recall"] > 0


# ---- 4. C = N against the exhaustive truth -----------------------------------------------------------------------------------------------------
def test_every_item_a_candidate_gives_the_exhaustive_counts():
    n = C = 101
    t, v, tm, vm = _samples(7, n)
    v[17], vm[17] = v[16], vm[16]                    # two identical videos: exact ties
    m = _model()
    td, vd, tmd, vmd = t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float()
    t2v, v2t = evaluator.two_stage_evaluation(m, td, vd, tmd, vmd, ARGS, C)
    assert t2v["cand_recall"] == 100.0 and v2t["cand_recall"] == 100.0 and "MR" in t2v and "MR" in v2t
    vi, ti = search.GalleryIndex(m, vd, vmd, "video"), search.GalleryIndex(m, td, tmd, "text")
    S = R.similarity(t, tm, ti.items.w.cpu(), v, vm, vi.items.w.cpu()).numpy()      # fp64, with the token weights the GPU used
    S[:, 17] = S[:, 16]                                                              # the same video twice
    gt = np.arange(n)
    for index, q, qm, S_dir, name in ((vi, td, tmd, S, "t2v"), (ti, vd, vmd, S.T, "v2t")):
        cand, fine = index.candidates(q, qm, C)
        assert np.array_equal(cand.cpu().numpy(), np.tile(np.arange(n), (n, 1)))
        found, greater, equal = evaluator.two_stage_counts(cand.cpu().numpy(), fine.cpu().numpy(), gt)
        assert found.all()
        left_out = 0
        for i in range(n):
            gaps = np.abs(S_dir[i] - S_dir[i, i])
            if np.any((gaps > 0) & (gaps <= 4e-6)):
                left_out += 1
                continue
            assert (greater[i], equal[i]) == (int((S_dir[i] > S_dir[i, i]).sum()), int((S_dir[i] == S_dir[i, i]).sum())), (name, i)
        print(f"{name}: {left_out} of {n} queries left out by the 4e-6 gap rule")
        assert left_out <= 0.05 * n
        if name == "t2v":
            assert equal[16] == 2 and equal[17] == 2                                 # the planted duplicate


# ---- 5. two gloo ranks on one card ----------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    args = SimpleNamespace(world_size=world, local_rank=rank)
    t, v, tm, vm = (x.to(DEV) for x in _samples(4242, N))
    res = evaluator.two_stage_evaluation(_model(), t, v, tm, vm, args, 8)
    torch.save(res, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_give_the_single_process_dictionaries(tmp_path):
    import torch.multiprocessing as mp
    t, v, tm, vm = (x.to(DEV) for x in _samples(4242, N))
    want = evaluator.two_stage_evaluation(_model(), t, v, tm, vm, ARGS, 8)
    world, port = 2, 29723
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        got = torch.load(f"{out}.{r}", weights_only=False)
        assert got[0] == want[0] and got[1] == want[1], r


# ---- 6. the exhaustive mode -------------------------------------------------------------------------------------------------------------------------
def test_no_candidates_means_the_exhaustive_lists():
    k = 10
    t, v, tm, vm = (x.to(DEV) for x in _samples(4242, N))
    tm, vm = tm.float(), vm.float()
    m = _model()
    ri, rv, ci, cv = evaluator.sharded_topk(m, t, v, tm, vm, k, ARGS)
    idx, val = search.GalleryIndex(m, v, vm, "video").search(t, tm, k, 0)
    assert torch.equal(idx, ri) and torch.equal(val.view(torch.int32), rv.view(torch.int32))
    idx, val = search.GalleryIndex(m, t, tm, "text").search(v, vm, k, 0)
    assert torch.equal(idx, ci) and torch.equal(val.view(torch.int32), cv.view(torch.int32))


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------------------------
def test_main_retrieval_logs_two_stage_only_with_the_flag():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--synthetic_test", "203"]
    outs = []
    for extra in ([], ["--rerank_top", "8"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()])
    plain, two = outs
    assert not any("two-stage" in line for line in plain)
    tagged = [line for line in two if "[two-stage C=8]" in line]
    assert len(tagged) == 3
    assert tagged[0].startswith("text->video [two-stage C=8] R@1") and "candidate recall" in tagged[0] and "R@10" not in tagged[0]
    assert tagged[1].startswith("video->text [two-stage C=8] R@1") and "candidate recall" in tagged[1]
    assert tagged[2].startswith("[two-stage C=8] wall time")
    assert [line for line in two if "two-stage" not in line] == plain
