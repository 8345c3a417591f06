"""GPU: the inverted-file prefilter of two-stage retrieval.  nr_ivf_list_sums against the float32 loop; the
invariants of build_ivf; nr_ivf_scan against nr_gemm_nt_f32 bit for bit, slot by slot; nr_ivf_select against the restatement of
tests/ivf_ref.py; the pipeline against the masked exact prefilter; P = L against the calls without an index; the evaluation, two
gloo ranks and the command line."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ivf_ref as I
from neighborretr_amd import evaluator, hip, modeling, ops, search, synth
from util import params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
N, Nt, Nv = 203, 24, 12             # the gallery of test_rerank_gpu.py: no multiple of a tile or of the rank count
NQ = 37                             # two full 16-query tiles and a ragged one
ARGS = SimpleNamespace(world_size=1)
_SCENE = {}


def _model():
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    return m.to(DEV).eval()


def _samples(seed, n):
    t, v, tm, vm = (torch.from_numpy(a) for a in synth.make_samples(seed, "test", n, Nt, Nv))
    v[17], vm[17] = v[16], vm[16]                  # two pairs of identical videos: exact ties of the coarse and the fine score
    v[101], vm[101] = v[100], vm[100]
    vm[2] = 0                                       # a fully masked video: the zero pooled vector
    return t, v, tm, vm


def _scene():
    """Built once: the model, the test set on the device, the video index, its prepared queries (the first NQ texts, the last one a
    repeat of text 5) and a querybank (texts, mask, videos, mask) for norm=."""
    if not _SCENE:
        t, v, tm, vm = (x.to(DEV) for x in _samples(4242, N))
        tm, vm = tm.float(), vm.float()
        m = _model()
        q, qm = t[:NQ].clone(), tm[:NQ].clone()
        q[NQ - 1], qm[NQ - 1] = q[5], qm[5]
        with torch.no_grad():
            qs = search._Side(m, q, qm, "text")
        bt, bv, btm, bvm = (torch.from_numpy(a).to(DEV) for a in synth.make_samples(77, "test", 40, Nt, Nv))
        _SCENE.update(m=m, t=t, v=v, tm=tm, vm=vm, q=q, qm=qm, qs=qs, bank=(bt, btm.float(), bv, bvm.float()), index={})
    return SimpleNamespace(**_SCENE)


def _index(L, iters=10, seed=0):
    s = _scene()
    key = (L, iters, seed)
    if key not in s.index:
        s.index[key] = search.GalleryIndex(s.m, s.v, s.vm, "video").build_ivf(L, iters, seed)
    return s.index[key]


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32).numpy()


def _bare(x):
    """A GalleryIndex that holds pooled vectors only: what build_ivf reads."""
    index = object.__new__(search.GalleryIndex)
    index.items = SimpleNamespace(n=x.shape[0], d=x.shape[1], pooled=x)
    index.ivf = None
    return index


def _item_lists(ivf):
    """list [N] of every gallery item, from the stored layout."""
    offsets, items = ivf.list_offsets.cpu().numpy(), ivf.list_items.cpu().numpy()
    lists = np.empty(len(items), dtype=np.int64)
    for l in range(len(offsets) - 1):
        lists[items[offsets[l]:offsets[l + 1]]] = l
    return lists


# ---- 1. nr_ivf_list_sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 512])
def test_list_sums_are_the_float32_loop(d):
    g = torch.Generator().manual_seed(d)
    x = torch.randn(N, d, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    x[7] = 0
    L = 9
    lists = torch.randint(0, L, (N,), generator=g).numpy()
    lists[lists == 4] = 5                           # list 4 is empty
    lists[:3] = 8
    items, offsets = I.layout(lists, L)
    sums = ops.ivf_list_sums(x.to(DEV), torch.from_numpy(items).to(DEV), torch.from_numpy(offsets).to(DEV))
    want = I.list_sums(x.numpy(), items, offsets)
    assert np.array_equal(_bits(sums), want.view(np.int32)) and not want[4].any() and sums.shape == (L, d)
    if d % 256 == 0:                                # nr_prepare_tokens takes widths that are multiples of 256
        unit = (sums / ops.prepare_tokens(sums, None, want_lo=False).norm[:, None]).cpu().numpy()
        s64 = np.stack([x.double().numpy()[items[offsets[l]:offsets[l + 1]]].sum(0) for l in range(L)])
        keep = np.arange(L) != 4
        worst = float(np.abs(unit[keep] - s64[keep] / np.linalg.norm(s64[keep], axis=1, keepdims=True)).max())
        print(f"max |centroid - fp64| = {worst:.3e} (bound 2e-6)")
        assert worst < 2e-6


def test_an_empty_list_and_a_list_of_zero_vectors_keep_their_centroid():
    n, d, L, seed = 12, 256, 3, 3
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(1)).abs()              # every pair of items scores > 0
    x = x / x.norm(dim=1, keepdim=True)
    x[perm[0]] = 0                                  # centroid 0 is the zero vector: only zero vectors tie their way into list 0
    x[perm[5]] = 0
    x[perm[2]] = x[perm[1]]                         # centroid 2 repeats centroid 1: every tie goes to list 1, list 2 stays empty
    xd = x.to(DEV)
    start = _bare(xd).build_ivf(L, iters=0, seed=seed).ivf
    assert np.array_equal(_bits(start.centroids), _bits(x[perm[:L]]))
    assert start.sizes == [2, n - 2, 0] and sorted(start.list_items[:2].tolist()) == sorted([int(perm[0]), int(perm[5])])
    ivf = _bare(xd).build_ivf(L, iters=1, seed=seed).ivf
    assert not _bits(ivf.centroids[0]).any()                                             # the zero sum kept the (zero) centroid
    assert np.array_equal(_bits(ivf.centroids[2]), _bits(x[perm[1]]))                    # the empty list kept its centroid
    assert not np.array_equal(_bits(ivf.centroids[1]), _bits(x[perm[1]]))                # list 1 moved to its members' mean
    assert abs(float(ivf.centroids[1].norm()) - 1) < 1e-6
    assert sum(ivf.sizes) == n and ivf.list_offsets.tolist()[-1] == n


# ---- 2. the invariants of the build ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,iters", [(7, 10), (13, 10), (7, 0), (1, 2), (N, 1)])
def test_build_invariants(L, iters):
    index = _index(L, iters)
    ivf, x = index.ivf, index.items.pooled
    assert not x[2].any()                                                                 # the masked item's pooled vector
    items, offsets = ivf.list_items.cpu().numpy(), ivf.list_offsets.cpu().numpy()
    assert ivf.list_items.dtype == torch.int32 and ivf.list_offsets.dtype == torch.int32
    assert sorted(items.tolist()) == list(range(N)) and offsets[0] == 0 and offsets[-1] == N and len(offsets) == L + 1
    assert np.all(np.diff(offsets) >= 0) and np.diff(offsets).tolist() == ivf.sizes and ivf.sizes_desc == sorted(ivf.sizes, reverse=True)
    for l in range(L):
        assert np.all(np.diff(items[offsets[l]:offsets[l + 1]]) > 0), l                    # ascending inside a list
    assert np.array_equal(_bits(ivf.pooled_sorted), _bits(x)[items])
    assert ivf.centroids.shape == (L, x.shape[1])
    top = ops.slab_topk_rows(ops.gemm_nt_f32(x, ivf.centroids), 1)[0][:, 0].clamp(min=0).cpu().numpy()
    assert np.array_equal(top, _item_lists(ivf))                                          # every item lies in its arg-max list
    assert _item_lists(ivf)[2] == 0                                                       # the zero vector: list 0
    assert _item_lists(ivf)[16] == _item_lists(ivf)[17] and _item_lists(ivf)[100] == _item_lists(ivf)[101]
    s = _scene()
    again = search.GalleryIndex(s.m, s.v, s.vm, "video").build_ivf(L, iters, 0, chunk=50).ivf       # the same seed: the same bits
    assert np.array_equal(_bits(again.centroids), _bits(ivf.centroids)) and torch.equal(again.list_items, ivf.list_items)
    assert torch.equal(again.list_offsets, ivf.list_offsets) and again.sizes == ivf.sizes
    if iters == 0:
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
        assert np.array_equal(_bits(ivf.centroids), _bits(x)[perm[:L].numpy()])
    if L == 7 and iters == 10:
        other = search.GalleryIndex(s.m, s.v, s.vm, "video").build_ivf(L, iters, 1).ivf
        assert not torch.equal(other.list_items, ivf.list_items)                          # another seed: another index
        index.attach_querybank(*s.bank[:2])                                               # the two attachments do not disturb each other
        assert index.ivf is ivf and index.norm is not None
        assert index.build_ivf(L, iters, 0).norm is not None and torch.equal(index.ivf.list_items, ivf.list_items)


# ---- 3. nr_ivf_scan, called directly --------------------------------------------------------------------------------------------------
def _scan_case(d):
    g = torch.Generator().manual_seed(900 + d)
    x = torch.randn(N, d, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    q = torch.randn(NQ, d, generator=g)
    q[NQ - 1] = q[5]
    L = 7
    lists = torch.randint(0, L, (N,), generator=g).numpy()
    lists[lists == 3] = 6                           # list 3 is empty
    items, offsets = I.layout(lists, L)
    return x, q, items, offsets


def _check_scan(x, q, items, offsets, probes, extra):
    sizes = np.diff(offsets)
    P = probes.shape[1]
    stride = int(np.sort(sizes)[::-1][:P].sum()) + extra
    xd, qd = x.to(DEV), q.to(DEV)
    rows = xd[torch.from_numpy(items).long().to(DEV)].contiguous()
    coarse = _bits(ops.gemm_nt_f32(qd, xd))
    score = torch.full((NQ, stride), float("nan"), device=DEV).view(torch.int32).fill_(0x7FC12345).view(torch.float32)
    item = torch.full((NQ, stride), -7, dtype=torch.int32, device=DEV)
    length = torch.full((NQ,), -7, dtype=torch.int32, device=DEV)
    out = ops.ivf_scan(qd, rows, torch.from_numpy(items).to(DEV), torch.from_numpy(offsets).to(DEV), torch.from_numpy(probes).to(DEV),
                       stride, int(sizes.max()), out=(score, item, length))
    assert out[0] is score and out[1] is item and out[2] is length
    score, item, length = _bits(score), item.cpu().numpy(), length.cpu().numpy()
    for i in range(NQ):
        want, base = I.pool(probes[i], items, offsets)
        n = len(want)
        assert length[i] == n == sum(sizes[p] for p in probes[i] if 0 <= p < len(sizes)), i
        assert np.array_equal(item[i, :n], want), i                                       # the probed lists in probe order
        assert np.array_equal(score[i, :n], coarse[i, want]), i                           # the bits of nr_gemm_nt_f32
        assert np.all(score[i, n:] == 0x7FC12345) and np.all(item[i, n:] == -7), i        # nothing written past the pool
    assert np.array_equal(score[NQ - 1], score[5]) and np.array_equal(item[NQ - 1], item[5])       # a repeated query: the same line
    fresh = ops.ivf_scan(qd, rows, torch.from_numpy(items).to(DEV), torch.from_numpy(offsets).to(DEV), torch.from_numpy(probes).to(DEV),
                         stride, N)                                                        # its own buffers, a looser size bound
    assert np.array_equal(fresh[2].cpu().numpy(), length)
    for i in range(NQ):
        assert np.array_equal(_bits(fresh[0])[i, :length[i]], score[i, :length[i]]), i
    return length


@pytest.mark.parametrize("d", [64, 128, 512])
def test_scan_fills_the_pools_with_the_bits_of_the_gemm(d):
    x, q, items, offsets = _scan_case(d)
    # list 0: 17 queries (a full tile and one more), list 1: 16, list 2: 4, list 4: one query, list 5: 36 (16 + 16 + 4), the empty
    # list 3 in the MIDDLE of every probe order, list 6 never probed
    probes = np.zeros((NQ, 3), dtype=np.int32)
    probes[:16, 0], probes[16:32, 0], probes[32:36, 0] = 0, 1, 2
    probes[:, 1] = 3
    probes[:, 2] = 5
    probes[0, 2] = 4
    probes[NQ - 1] = probes[5]
    counts = np.bincount(probes.reshape(-1), minlength=7)
    assert counts.tolist() == [17, 16, 4, NQ, 1, 36, 0] and offsets[4] == offsets[3]
    length = _check_scan(x, q, items, offsets, probes, extra=5)
    assert length.min() > 0
    # missing probes (-1), also at the LAST rank, and an index past the lists: empty lists; every query probes list 6 first
    probes = np.full((NQ, 2), 6, dtype=np.int32)
    probes[0::2, 1], probes[1::2, 1] = -1, 2
    probes[3, 1] = 7
    probes[NQ - 1] = probes[5]
    _check_scan(x, q, items, offsets, probes, extra=0)
    # one probe per query: only empty lists for the first queries (pool_len 0)
    probes = np.full((NQ, 1), 1, dtype=np.int32)
    probes[:20, 0] = 3
    probes[NQ - 1] = probes[5]
    length = _check_scan(x, q, items, offsets, probes, extra=0)
    assert length[:20].tolist() == [0] * 20


# ---- 4. nr_ivf_select, called directly --------------------------------------------------------------------------------------------------
def _select_pools(n, stride, lengths, seed):
    """Pool lines full of ties: scores from a handful of values with both zeros and both infinities, a NaN per line, distinct
    items in random order, a descending run at the front; every line filled to `stride` (the tail must be ignored)."""
    g = np.random.default_rng(seed)
    values = np.asarray([0.0, -0.0, 0.25, 0.25, 0.5, -0.5, np.inf, -np.inf, 0.7071], dtype=np.float32)
    score = values[g.integers(0, len(values), (n, stride))]
    item = np.stack([g.permutation(4 * stride)[:stride] for _ in range(n)]).astype(np.int32)
    item[:, :8] = np.sort(item[:, :8], axis=1)[:, ::-1]                                   # equal scores at descending item order
    score[:, :8] = 0.5
    score[np.arange(n), g.integers(0, stride, n)] = np.nan
    score[:, -1] = np.inf                                                                 # past most lines' length: never taken there
    return score, item, np.asarray(lengths, dtype=np.int32)


def _check_select(score, item, length, C):
    cand, out = ops.ivf_select(torch.from_numpy(score).to(DEV), torch.from_numpy(item).to(DEV), torch.from_numpy(length).to(DEV), C,
                               want_score=True)
    only = ops.ivf_select(torch.from_numpy(score).to(DEV), torch.from_numpy(item).to(DEV), torch.from_numpy(length).to(DEV), C)
    assert torch.equal(only, cand)
    cand, out = cand.cpu().numpy(), _bits(out)
    for i in range(len(length)):
        want_c, want_s = I.select(score[i], item[i], int(length[i]), C)
        assert np.array_equal(cand[i], want_c), (i, int(length[i]))
        assert np.array_equal(out[i], want_s.view(np.int32)), (i, int(length[i]))


@pytest.mark.parametrize("C", [1, 16, 128])
def test_select_equals_the_restatement(C):
    stride = 300
    lengths = [0, 1, max(C - 1, 0), C, C + 1, 299, 300, 8, 9]
    score, item, length = _select_pools(len(lengths), stride, lengths, C)
    score[4, :C + 1] = 0.25                                                               # one line of C + 1 equal scores
    _check_select(score, item, length, C)
    nan = np.full((2, 5), np.nan, dtype=np.float32)                                       # only NaNs; NaNs reaching into the top C
    nan[1, 2] = 1.0
    _check_select(nan, np.tile(np.arange(5, dtype=np.int32)[::-1], (2, 1)).copy(), np.asarray([5, 5], dtype=np.int32), C)


@pytest.mark.parametrize("stride,C", [(hip.IVF_CACHE_KEYS + 1, 16), (hip.IVF_CACHE_KEYS, 128)])
def test_select_at_the_edge_of_the_key_cache(stride, C):
    """One line just past the longest that keeps its keys in LDS (it re-reads memory in every pass), and the longest that does."""
    score, item, length = _select_pools(2, stride, [stride, stride - 3], stride)
    _check_select(score, item, length, C)


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------------------
def _masked_exact(index, qs, P, C):
    """Consequence 1 on the GPU's own numbers: the exact prefilter (coarse_scores + slab_topk_rows) on the coarse matrix with the
    entries outside every query's pool at -inf; a pick that is outside the pool is dropped.  -> (cand, pool_len)."""
    ivf = index.ivf
    probes = ops.slab_topk_rows(ops.gemm_nt_f32(qs.pooled, ivf.centroids), P)[0].cpu().numpy()
    lists = _item_lists(ivf)
    inside = torch.from_numpy((lists[None, :, None] == probes[:, None, :]).any(axis=2)).to(DEV)
    coarse = index.coarse_scores(qs.pooled)
    idx, _ = ops.slab_topk_rows(torch.where(inside, coarse, torch.full_like(coarse, float("-inf"))), C)
    ok = (idx >= 0) & torch.gather(inside, 1, idx.clamp(min=0).long())
    big = torch.iinfo(torch.int32).max
    idx = torch.where(ok, idx, torch.full_like(idx, big)).sort(dim=1).values
    return torch.where(idx == big, torch.full_like(idx, -1), idx), inside.sum(dim=1).to(torch.int32)


@pytest.mark.parametrize("L", [7, 13])
def test_candidates_equal_the_masked_exact_prefilter(L):
    s = _scene()
    index = _index(L)
    g = index.items
    short = 0
    for P in (1, 3, L):
        for C in (1, 16, 128):
            cand, fine = index.candidates(s.q, s.qm, C, nprobe=P)
            want, pool_len = _masked_exact(index, s.qs, P, C)
            assert torch.equal(cand, want), (P, C)
            want_fine = ops.local_level_cand(s.qs.prep, g.prep, s.qs.w, g.w, NQ, s.qs.n_tok, g.n, g.n_tok, want, hip.PREC_BF16X3)
            assert np.array_equal(_bits(fine), _bits(want_fine)), (P, C)
            assert torch.equal((cand >= 0).sum(dim=1).to(torch.int32), pool_len.clamp(max=C)), (P, C)
            short += int((pool_len < C).sum())
            same, _, stats = index.candidates(s.q, s.qm, C, nprobe=P, ivf_stats=True)
            assert torch.equal(same, cand) and torch.equal(stats[:, 0], pool_len)
            exact = index.candidates(s.q, s.qm, C)[0]
            assert torch.equal(stats[:, 2], (exact >= 0).sum(dim=1).to(torch.int32))
            kept = [len(set(e[e >= 0].tolist()) & set(c.tolist())) for e, c in zip(exact.cpu().numpy(), cand.cpu().numpy())]
            assert stats[:, 1].tolist() == kept
            assert torch.equal(cand[NQ - 1], cand[5])                                     # the repeated query
    assert short > 0                                                                      # pools shorter than C did occur
    # the planted ties: where one of two identical videos is a candidate next to a cut at its score, the lower index is taken
    cand = index.candidates(s.q, s.qm, 16, nprobe=L)[0].cpu().numpy()
    for lo, hi in ((16, 17), (100, 101)):
        assert not np.any((cand == hi).any(1) & ~(cand == lo).any(1))
    a = index.candidates(s.q, s.qm, 16, chunk=7, nprobe=3)
    b = index.candidates(s.q, s.qm, 16, chunk=256, nprobe=3)
    assert torch.equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))           # the lists do not depend on the chunk
    c = index.candidates(s.q[30:], s.qm[30:], 16, nprobe=3)                               # ... nor on who shares the batch
    assert torch.equal(c[0], b[0][30:]) and np.array_equal(_bits(c[1]), _bits(b[1])[30:])


@pytest.mark.parametrize("L", [7, 13])
def test_probing_every_list_is_the_exact_prefilter(L):
    s = _scene()
    index = _index(L)
    if index.norm is None:
        index.attach_querybank(*s.bank[:2])
    for C in (1, 16, 128):
        got, want = index.candidates(s.q, s.qm, C, nprobe=L), index.candidates(s.q, s.qm, C)
        assert torch.equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), C
    k, C = 5, 16
    got, want = index.search(s.q, s.qm, k, C, nprobe=L, return_candidates=True), index.search(s.q, s.qm, k, C, return_candidates=True)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want)) and len(got) == len(want) == 4
    for norm in ("qbnorm", "is"):
        got = index.search(s.q, s.qm, k, C, nprobe=L, norm=norm, return_candidates=True)
        want = index.search(s.q, s.qm, k, C, norm=norm, return_candidates=True)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want)) and len(got) == len(want) == 5
        got, want = index.candidates(s.q, s.qm, C, norm=norm, nprobe=L), index.candidates(s.q, s.qm, C, norm=norm)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want)) and len(got) == len(want) == 4
    # norm= on shorter pools: the lists of nprobe, then the one launch of 6.15 on them
    cand, fine = index.candidates(s.q, s.qm, C, nprobe=2)
    got = index.candidates(s.q, s.qm, C, norm="qbnorm", nprobe=2)
    _, _, corr, gate = ops.cand_norm_rerank(fine, cand, len(index), 1, norm=index.norm, active=index.active, beta=index.norm_beta)
    assert torch.equal(got[0], cand) and np.array_equal(_bits(got[2]), _bits(corr)) and torch.equal(got[3], gate)
    empty = index.candidates(s.q[:0], s.qm[:0], C, nprobe=2, ivf_stats=True)
    assert empty[0].shape == (0, C) and empty[2].shape == (0, 3)


# ---- 6. the evaluation ------------------------------------------------------------------------------------------------------------------------
def test_evaluation_with_every_list_probed_is_todays_plus_the_new_fields():
    s = _scene()
    C, L = 8, 7
    want = evaluator.two_stage_evaluation(s.m, s.t, s.v, s.tm, s.vm, ARGS, C)
    got = evaluator.two_stage_evaluation(s.m, s.t, s.v, s.tm, s.vm, ARGS, C, n_lists=L, nprobe=L)
    for g, w in zip(got, want):
        assert {k: g[k] for k in w} == w and set(g) - set(w) == {"n_lists", "nprobe", "pool_mean", "ivf_overlap"}
        assert (g["n_lists"], g["nprobe"], g["pool_mean"], g["ivf_overlap"]) == (L, L, 1.0, 1.0)
    assert evaluator.two_stage_evaluation(s.m, s.t, s.v, s.tm, s.vm, ARGS, C, n_lists=0, nprobe=0) == want


def test_evaluation_equals_the_metrics_of_the_same_lists():
    s = _scene()
    C, L, P = 8, 7, 2
    got = evaluator.two_stage_evaluation(s.m, s.t, s.v, s.tm, s.vm, ARGS, C, n_lists=L, nprobe=P, hubness_k=4)
    gt = np.arange(N)
    sides = ((search.GalleryIndex(s.m, s.v, s.vm, "video"), s.t, s.tm), (search.GalleryIndex(s.m, s.t, s.tm, "text"), s.v, s.vm))
    for m, (index, q, qm) in zip(got, sides):
        cand, fine, stats = index.build_ivf(L, 10, 0).candidates(q, qm, C, nprobe=P, ivf_stats=True)
        want = evaluator.two_stage_metrics(*evaluator.two_stage_counts(cand.cpu().numpy(), fine.cpu().numpy(), gt), C)
        assert {k: m[k] for k in want} == want and "hubness" in m
        exact = index.candidates(q, qm, C)[0].cpu().numpy()
        assert m["ivf_overlap"] == pytest.approx(I.overlap(exact, cand.cpu().numpy()), abs=1e-12) and 0 < m["ivf_overlap"] < 1
        assert m["pool_mean"] == pytest.approx(float(stats[:, 0].double().mean()) / N, abs=1e-12) and 0 < m["pool_mean"] < 1
        assert (m["n_lists"], m["nprobe"]) == (L, P)
    plain = evaluator.two_stage_evaluation(s.m, s.t, s.v, s.tm, s.vm, ARGS, C, n_lists=L, nprobe=P, norm="is", querybank=s.bank)
    assert plain[0]["normalised"]["label"] == "[two-stage C=8 IS b=20]" and plain[0]["ivf_overlap"] == got[0]["ivf_overlap"]
    assert {k: plain[0][k] for k in ("R1", "R5", "cand_recall", "cols")} == {k: got[0][k] for k in ("R1", "R5", "cand_recall", "cols")}


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    args = SimpleNamespace(world_size=world, local_rank=rank)
    t, v, tm, vm = (x.to(DEV) for x in _samples(4242, N))
    res = evaluator.two_stage_evaluation(_model(), t, v, tm, vm, args, 8, n_lists=7, nprobe=2)
    torch.save(res, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_give_the_single_process_dictionaries(tmp_path):
    import torch.multiprocessing as mp
    s = _scene()
    want = evaluator.two_stage_evaluation(s.m, s.t, s.v, s.tm, s.vm, ARGS, 8, n_lists=7, nprobe=2)
    world, port = 2, 29741
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        got = torch.load(f"{out}.{r}", weights_only=False)
        assert got[0] == want[0] and got[1] == want[1], r


def test_main_retrieval_logs_the_inverted_file_only_with_the_flags():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--synthetic_test", "203",
           "--rerank_top", "8"]
    outs = []
    for extra in ([], ["--rerank_lists", "4", "--rerank_probe", "2"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()])
    plain, ivf = outs
    # without the two flags: the lines of test_rerank_gpu.py, nothing of the inverted file
    assert not any("IVF" in line or "exact prefilter" in line for line in plain)
    tagged = [line for line in plain if "two-stage" in line]
    assert len(tagged) == 3 and all("[two-stage C=8]" in line for line in tagged) and tagged[2].startswith("[two-stage C=8] wall time")
    tag = "[two-stage C=8 IVF L=4 P=2]"
    tagged = [line for line in ivf if "two-stage" in line]
    assert len(tagged) == 5 and all(tag in line for line in tagged)
    assert tagged[0].startswith(f"text->video {tag} R@1") and "candidate recall" in tagged[0]
    assert tagged[1].startswith(f"text->video {tag} pool ") and tagged[1].endswith("% of the exact prefilter's candidates")
    assert tagged[2].startswith(f"video->text {tag} R@1") and tagged[3].startswith(f"video->text {tag} pool ")
    assert tagged[4].startswith(f"{tag} wall time")
    assert [line for line in ivf if "two-stage" not in line] == [line for line in plain if "two-stage" not in line]
