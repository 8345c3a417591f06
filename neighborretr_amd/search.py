"""Two-stage retrieval: a pooled single-vector prefilter picks C candidates per query, the fused token-level score
(nr_local_level_cand) re-ranks those candidates only.

The reference has no such path: it scores every (text, video) pair (training/evaluator.py:21-63).  Here a gallery is
prepared ONCE (GalleryIndex: bf16 hi/lo tokens, token weights, pooled vectors) and searched by any number of query batches.

  coarse score   p_q . p_g,   p(x) = normalize(sum_tok w[tok] x^[tok])   -- the fine score with both max-pools relaxed to
                 weighted means; x^ = the normalised, masked tokens, w = the scorer weights of the fine stage
  candidates     the top C of every coarse row (ops.slab_topk_rows: score descending, ties by lower index), then sorted by
                 ascending gallery index, so that position order equals index order
  fine score     ops.local_level_cand on the split-bf16 plan, for the candidates only
  result         the top k of the fine scores, ties by lower gallery index

The coarse scores are computed in row chunks ([chunk, N], dropped after use): nothing of size n x N is ever allocated.  Every
step is deterministic per element (pointwise torch ops, this library's own kernels), so a query's list and scores do not depend
on the chunk size or on which other queries share its batch.

Query-bank normalisation: `attach_querybank` computes, once per gallery, every item's normaliser and the activation
set from a bank of training queries; `candidates` / `search` with norm="is" | "qbnorm" then correct every query's candidate scores and
re-rank them in one launch (nr_cand_norm_rerank).  Without the argument nothing changes.

Inverted-file prefilter: `build_ivf` deals the gallery's pooled vectors to L k-means lists, once per gallery;
`candidates` / `search` with nprobe=P then score a query against the members of the P lists whose centroids it is closest to
(nr_ivf_scan) and take the candidates from that pool (nr_ivf_select) -- exactly the lists the exact prefilter selects from a
coarse matrix whose entries outside the pool are -inf, and with P = L exactly today's.  Without the argument nothing changes.

Local scaling: `attach_localscale` computes, once per gallery, every item's k-nearest-neighbourhood statistics
against a bank of training queries; `candidates` / `search` with local_scaling="csls" | "nicdm" | "ls" then take every query's own
statistics from its candidates' fine scores, correct the scores and re-rank them in one launch (nr_cand_localscale_rerank).
Without the argument nothing changes.

Mutual proximity: `attach_mutualprox` keeps, once per gallery, every item's line of scores against a bank of
training queries, its non-NaN count and its moments; `candidates` / `search` with mutual_proximity="emp" | "gauss" then take every
query's own line among its candidates' fine scores, correct the scores and re-rank them in one launch (nr_cand_mutualprox_rerank).
Without the argument nothing changes.
"""
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional

import torch

from . import head, hip, ops

MAX_CANDIDATES = 128                      # nr_local_level_cand: C <= 128 (= hip.TOPK_MAX, the longest top-k list)
_SCORER = {"video": "video_weight_fc", "text": "text_weight_fc"}
NORM_MODES = ("is", "qbnorm")             # query-bank normalisation of the candidate scores
LOCAL_SCALING_MODES = ("csls", "nicdm", "ls")       # local scaling of the candidate scores
MUTUAL_PROXIMITY_MODES = ("emp", "gauss")           # mutual proximity of the candidate scores


def _int_in(x, lo=None, hi=None):
    """x is an int, not a bool, with lo <= x <= hi (None: no bound)."""
    return isinstance(x, int) and not isinstance(x, bool) and (lo is None or lo <= x) and (hi is None or x <= hi)


def check_candidates(n_candidates, allow_zero=False):
    """n_candidates as an int in [1, 128] (allow_zero: 0 = the exhaustive path)."""
    lo = 0 if allow_zero else 1
    if not _int_in(n_candidates, lo, MAX_CANDIDATES):
        raise ValueError(f"n_candidates must be an integer in [{lo}, {MAX_CANDIDATES}], got {n_candidates!r}")
    return int(n_candidates)


def check_chunk(chunk):
    if not _int_in(chunk, 1):
        raise ValueError(f"chunk must be an integer >= 1, got {chunk!r}")
    return int(chunk)


def check_ivf_build(n_lists, iters, seed, n_items):
    """(n_lists, iters, seed) of build_ivf as ints: 1 <= n_lists <= n_items, iters >= 0, any integer seed."""
    if not _int_in(n_lists, 1, n_items):
        raise ValueError(f"n_lists must be an integer in [1, {n_items}] (the gallery's size), got {n_lists!r}")
    if not _int_in(iters, 0):
        raise ValueError(f"iters must be an integer >= 0, got {iters!r}")
    if not _int_in(seed):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    return int(n_lists), int(iters), int(seed)


def check_nprobe(nprobe, n_lists):
    """nprobe as an int in [1, min(n_lists, 128)]."""
    hi = min(int(n_lists), hip.IVF_MAX_PROBE)
    if not _int_in(nprobe, 1, hi):
        raise ValueError(f"nprobe must be an integer in [1, min(n_lists, {hip.IVF_MAX_PROBE}) = {hi}], got {nprobe!r}")
    return int(nprobe)


def check_norm(norm):
    """norm as None, "is" or "qbnorm" ("dsl" needs the query's whole row of scores: the evaluator's exhaustive path has it)."""
    if norm is not None and norm not in NORM_MODES:
        raise ValueError(f"norm must be None or one of {NORM_MODES}, got {norm!r}")
    return norm


def check_local_scaling(mode):
    """local_scaling as None, "csls", "nicdm" or "ls"."""
    if mode is not None and (not isinstance(mode, str) or mode not in LOCAL_SCALING_MODES):
        raise ValueError(f"local_scaling must be None or one of {LOCAL_SCALING_MODES}, got {mode!r}")
    return mode


def check_local_scaling_k(k):
    """The neighbourhood size of local scaling as an int in [1, 128]."""
    if not _int_in(k, 1, hip.TOPK_MAX):
        raise ValueError(f"local scaling k must be an integer in [1, {hip.TOPK_MAX}], got {k!r}")
    return int(k)


def check_correction(norm, local_scaling):
    """(norm, local_scaling) as check_norm and check_local_scaling take them, at most one of them set: both correct the scores."""
    norm, local_scaling = check_norm(norm), check_local_scaling(local_scaling)
    if norm is not None and local_scaling is not None:
        raise ValueError(f"local_scaling={local_scaling!r} and norm={norm!r} both correct the candidate scores: choose one")
    return norm, local_scaling


def check_mutual_proximity(mode):
    """mutual_proximity as None, "emp" or "gauss"."""
    if mode is not None and (not isinstance(mode, str) or mode not in MUTUAL_PROXIMITY_MODES):
        raise ValueError(f"mutual_proximity must be None or one of {MUTUAL_PROXIMITY_MODES}, got {mode!r}")
    return mode


def check_corrections(norm, local_scaling, mutual_proximity):
    """(norm, local_scaling, mutual_proximity) as their own checks take them, at most one of them set: each corrects the scores."""
    norm, local_scaling = check_correction(norm, local_scaling)
    mutual_proximity = check_mutual_proximity(mutual_proximity)
    for name, other in (("norm", norm), ("local_scaling", local_scaling)):
        if mutual_proximity is not None and other is not None:
            raise ValueError(f"mutual_proximity={mutual_proximity!r} and {name}={other!r} both correct the candidate scores: choose one")
    return norm, local_scaling, mutual_proximity


def _check_tokens(feat, mask, what):
    if not torch.is_tensor(feat) or feat.dim() != 3:
        raise ValueError(f"{what} features must be a [n, tokens, d] tensor")
    if not torch.is_tensor(mask) or mask.dim() != 2 or tuple(mask.shape) != tuple(feat.shape[:2]):
        raise ValueError(f"{what} mask must be [n, tokens] = {tuple(feat.shape[:2])}")


class CandCorrection(NamedTuple):
    """One correction of candidate scores, in the manner of evaluator.Correction: what `candidates` / `search` need to know of it."""
    name: str                                 # the argument of candidates / search that carries its mode
    needs: str                                # the attribute of the index its attach_* sets: None = not attached
    missing: str                              # the refusal when it is not attached; {mode!r} is filled in
    min_candidates: Callable                  # index -> the smallest n_candidates it can work on
    too_few: Optional[str]                    # the refusal below that; {need} and {C} are filled in
    rerank: Callable                          # (index, mode, fine, cand, k) -> (idx, val, corr, extra): its ONE ops call


_NORM = CandCorrection(
    "norm", "norm", "norm={mode!r} needs the gallery's query-bank statistics: call attach_querybank(...) first", lambda index: 1, None,
    lambda index, mode, fine, cand, k: ops.cand_norm_rerank(
        fine, cand, len(index), k, norm=index.norm, active=index.active if mode == "qbnorm" else None, beta=index.norm_beta))
# the text side is the row of the formulas: the query for a video gallery, the gallery item for a text gallery
_LOCAL_SCALING = CandCorrection(
    "local_scaling", "ls_mean", "local_scaling={mode!r} needs the gallery's neighbourhood statistics: call attach_localscale(...) first",
    lambda index: index.ls_k, "local_scaling takes a query's neighbourhood of ls_k = {need} among its candidates: n_candidates >= {need} "
    "expected, got {C}", lambda index, mode, fine, cand, k: ops.cand_localscale_rerank(
        fine, cand, len(index), k, index.ls_kth if mode == "ls" else index.ls_mean, mode, index.ls_k, index.side == "video"))
# the formulas are symmetric in their two lines: neither side needs to know which one is the row
_MUTUAL_PROXIMITY = CandCorrection(
    "mutual_proximity", "mp_mean", "mutual_proximity={mode!r} needs the gallery's bank lines: call attach_mutualprox(...) first",
    lambda index: 1, None, lambda index, mode, fine, cand, k: ops.cand_mutualprox_rerank(
        fine, cand, len(index), k, mode, g_line=index.mp_line, g_cnt=index.mp_cnt, g_mean=index.mp_mean, g_sd=index.mp_sd))


def pooled_vectors(feat, mask, norm, w):
    """p [n, d] fp32 = normalize(sum_tok w[tok] x^[tok]); norm [n * tokens] = the token norms nr_prepare_tokens wrote.  A fully
    masked item gives the zero vector.  Pointwise ops and one prepare launch (the norm): the same bits for any batch."""
    n, n_tok, d = feat.shape
    m = mask.float()
    coef = torch.where(m > 0, w.view(n, n_tok), torch.zeros_like(m)) / norm.view(n, n_tok)
    u = torch.zeros((n, d), dtype=torch.float32, device=feat.device)
    for t in range(n_tok):
        u.addcmul_(feat[:, t, :], coef[:, t:t + 1])
    if n == 0:
        return u
    return u / ops.prepare_tokens(u, None, want_lo=False).norm[:, None]


class _Side:
    """One prepared token set: split-bf16 tokens, scorer weights, pooled vectors."""

    def __init__(self, model, feat, mask, side):
        feat = feat.float().contiguous()
        mask = mask.float().contiguous()
        self.n, self.n_tok, self.d = feat.shape
        if self.n:
            self.prep = ops.prepare_tokens(feat, mask, want_lo=True)
            self.w, _ = head.token_weights(self.prep, mask, model.scorer_weights(_SCORER[side]), self.n, self.n_tok, hip.PREC_BF16X3)
            self.pooled = pooled_vectors(feat, mask, self.prep.norm, self.w)
        else:
            self.prep = self.w = None
            self.pooled = torch.zeros((0, self.d), dtype=torch.float32, device=feat.device)


class GalleryIndex:
    """A gallery prepared once for two-stage search.  side="video": the items are videos, the queries texts; side="text":
    the items are texts, the queries videos (the fine score is symmetric in its two sides)."""

    def __init__(self, model, feat, mask, side="video"):
        if side not in _SCORER:
            raise ValueError(f"side must be 'video' or 'text', got {side!r}")
        _check_tokens(feat, mask, "gallery")
        if feat.shape[0] < 1:
            raise ValueError("the gallery is empty")
        self.model = model
        self.side = side
        self.query_side = "text" if side == "video" else "video"
        self.feat, self.mask = feat, mask
        with torch.no_grad():
            self.items = _Side(model, feat, mask, side)
        self.norm = self.active = self.norm_beta = self.qb_k = None
        self.n_bank = 0
        self.ivf = None
        self.ls_mean = self.ls_kth = self.ls_k = None
        self.ls_n_bank = 0
        self.mp_line = self.mp_cnt = self.mp_mean = self.mp_sd = None
        self.mp_n_bank = 0

    def __len__(self):
        return self.items.n

    def _bank_scores(self, bank_feat, bank_mask, chunk):
        """The bank x gallery similarity in the evaluator's orientation (texts are rows), after the bank and chunk are checked: Qt
        [M, N] for a video gallery, Qv [N, M] for a text gallery.  Scored once, whole; `chunk` only bounds the rows of one launch."""
        _check_tokens(bank_feat, bank_mask, "querybank")
        if bank_feat.shape[0] < 1:
            raise ValueError("the querybank is empty")
        if bank_feat.shape[2] != self.items.d:
            raise ValueError(f"the querybank is {bank_feat.shape[2]} wide, the gallery {self.items.d}")
        if bank_feat.device != self.feat.device or bank_mask.device != self.feat.device:
            raise ValueError("querybank and gallery must be on the same device")
        chunk = check_chunk(chunk)
        from .evaluator import _slab_similarity
        N, M = len(self), bank_feat.shape[0]
        bank_feat, bank_mask, feat, mask = bank_feat.float(), bank_mask.float(), self.feat.float(), self.mask.float()
        if self.side == "video":
            return _slab_similarity(self.model, bank_feat, feat, bank_mask, mask, 0, M, chunk)
        return _slab_similarity(self.model, feat, bank_feat, mask, bank_mask, 0, N, chunk)

    def attach_querybank(self, bank_feat, bank_mask, beta=20.0, qb_k=1, chunk=256):
        """The gallery's query-bank statistics, computed once -> self.  The bank holds items of
        `self.query_side` (texts for a video gallery, videos for a text gallery), [M, tokens, d] with a mask [M, tokens].
        Stores norm [N] fp32 (item j's normaliser: the log-sum-exp of beta x its scores against the M bank items), active [N]
        int32 (1 iff j is in the top-qb_k list of some bank item), norm_beta, qb_k and n_bank: the definitions of DESIGN.md 6.2
        in the evaluator's orientation (texts are rows), so at one rank these are the bits of the exhaustive `qbnorm`.
        Every argument is checked before any work.

        The bank product (bank x gallery similarity, 4 M N bytes: 41 MB at M = 512, N = 20 000) is scored once, whole, and
        dropped.  The statistics are never chunked over bank items: merging (max, sum) pairs is not associative bit for bit,
        so `norm` would depend on the chunk size (`chunk` only bounds the rows of one similarity launch)."""
        beta, qb_k = ops._check_beta(beta), ops._check_k(qb_k)
        with torch.no_grad():
            Q = self._bank_scores(bank_feat, bank_mask, chunk)
            N, M = len(self), bank_feat.shape[0]
            if self.side == "video":
                norm = ops.hubnorm_combine(ops.hubnorm_col_stats(Q, beta)[None])
                lists, _ = ops.slab_topk_rows(Q, qb_k)
            else:
                norm = ops.hubnorm_row_lse(Q, beta)
                lists, _ = ops.slab_topk_cols(Q, 0, qb_k)
            none = torch.zeros((M,), dtype=torch.int32, device=Q.device)
            occ, _ = ops.topk_occurrences(lists, N, none, none)
            self.norm, self.active = norm, (occ > 0).to(torch.int32)
        self.norm_beta, self.qb_k, self.n_bank = beta, qb_k, M
        return self

    def attach_localscale(self, bank_feat, bank_mask, k=10, chunk=256):
        """The gallery's neighbourhood statistics against a query bank, computed once -> self.  The bank holds
        items of `self.query_side`, as in attach_querybank.  Item j's neighbourhood is its top-k list among the M bank items
        (ops.slab_topk_cols of Qt [M, N] for a video gallery, ops.slab_topk_rows of Qv [N, M] for a text gallery); stores ls_mean
        [N] fp32 and ls_kth [N] fp32 (ops.localscale_stats: the list's mean and its last value; both are kept, so the mode is
        chosen at search time), ls_k and ls_n_bank.  These are the bits the exhaustive bank form (evaluator._local_scaling_stats
        with bank_slabs) computes for the columns (video gallery) or the rows (text gallery) at any world size.  Every argument is
        checked before any work; the bank product is scored once, whole, and dropped (`chunk` only bounds the rows of one
        similarity launch).  attach_querybank's and build_ivf's state is not touched."""
        k = check_local_scaling_k(k)
        with torch.no_grad():
            Q = self._bank_scores(bank_feat, bank_mask, chunk)
            lists = ops.slab_topk_cols(Q, 0, k) if self.side == "video" else ops.slab_topk_rows(Q, k)
            self.ls_mean, self.ls_kth = ops.localscale_stats(*lists)
        self.ls_k, self.ls_n_bank = k, bank_feat.shape[0]
        return self

    def attach_mutualprox(self, bank_feat, bank_mask, chunk=256):
        """The gallery's mutual-proximity lines against a query bank, computed once -> self.  The bank holds
        items of `self.query_side`, as in attach_querybank.  Stores mp_line [N, M] fp32, item-major: row j = the M bank scores of
        item j in bank order (Qt.T.contiguous() of Qt [M, N] for a video gallery, Qv [N, M] itself for a text gallery); mp_cnt [N]
        int32, the lines' non-NaN counts (ops.mp_line_counts); mp_mean, mp_sd [N] fp32, their moments (ops.mp_col_moments +
        ops.mp_moments_combine of Qt, ops.mp_row_moments of Qv: the bits the exhaustive `--mutual_proximity gauss
        --mutual_proximity_bank 1` has for those lines at one rank); mp_n_bank = M.  Both modes' state is kept, so the mode is
        chosen at search time.  The lines take 4 N M bytes: 41 MB at N = 20 000, M = 512, about 8 % of the prepared tokens.
        Every argument is checked before any work; the bank product is scored once, whole (`chunk` only bounds the rows of one
        similarity launch).  attach_querybank's, attach_localscale's and build_ivf's state is not touched."""
        if torch.is_tensor(bank_feat) and bank_feat.dim() == 3:
            ops._mp_line(bank_feat.shape[0], "attach_mutualprox")      # everything else is _bank_scores' to refuse
        with torch.no_grad():
            Q = self._bank_scores(bank_feat, bank_mask, chunk)
            M = bank_feat.shape[0]
            if self.side == "video":
                line = Q.T.contiguous()
                mean, sd = ops.mp_moments_combine(ops.mp_col_moments(Q)[None])
            else:
                line = Q
                mean, sd = ops.mp_row_moments(Q)
            cnt, _ = ops.mp_line_counts(R=line)
            self.mp_line, self.mp_cnt, self.mp_mean, self.mp_sd = line, cnt, mean, sd
        self.mp_n_bank = M
        return self

    def build_ivf(self, n_lists, iters=10, seed=0, chunk=256):
        """The inverted-file index of the gallery's pooled vectors, built once -> self.  n_lists = L k-means
        lists (1 <= L <= N), iters >= 0 rounds of assign + update, then one final assignment.  The initial centroids are
        x[perm[:L]], perm = torch.randperm(N) of a CPU generator seeded with `seed`: every rank builds the same index.
          assign   item g goes to argmax_l c_l . x_g (ops.gemm_nt_f32 in row chunks, ops.slab_topk_rows(., 1): ties to the lower
                   list, a zero vector to list 0)
          update   c_l = normalize(sum of the members of list l in ascending gallery index) (ops.ivf_list_sums, the norm of
                   ops.prepare_tokens as pooled_vectors takes it); an empty list, or one whose sum is the zero vector, keeps its
                   previous centroid
        Stores self.ivf: centroids [L, d], list_offsets [L + 1] int32, list_items [N] int32 (ascending inside a list, lists in
        order), pooled_sorted [N, d] = pooled[list_items], and on the host sizes (a list) and sizes_desc.  Every item lies in the
        list the assignment names for the STORED centroids.  The build reads the list sizes back (one synchronisation); a search
        never does.  Every argument is checked before any work; attach_querybank's statistics are not touched."""
        N, d = self.items.n, self.items.d
        L, iters, seed = check_ivf_build(n_lists, iters, seed, N)
        chunk = check_chunk(chunk)
        if d % 16 != 0:
            raise ValueError(f"the pooled vectors are {d} wide: the inverted file needs a multiple of 16")
        x = self.items.pooled
        dev = x.device
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
        lists = torch.arange(L + 1, dtype=torch.int32, device=dev)

        def assign(cent):
            a = torch.empty((N,), dtype=torch.int32, device=dev)
            for lo in range(0, N, chunk):
                a[lo:lo + chunk] = ops.slab_topk_rows(ops.gemm_nt_f32(x[lo:lo + chunk], cent), 1)[0][:, 0]
            ordered, items = torch.sort(a.clamp_(min=0), stable=True)      # a row of NaN scores names no list: list 0
            return items.to(torch.int32), torch.searchsorted(ordered, lists, out_int32=True)

        with torch.no_grad():
            cent = x[perm[:L].to(dev)].contiguous()
            for _ in range(iters):
                items, offsets = assign(cent)
                sums = ops.ivf_list_sums(x, items, offsets)
                new = sums / ops.prepare_tokens(sums, None, want_lo=False).norm[:, None]
                keep = (offsets[1:] == offsets[:-1]) | (sums == 0).all(dim=1)
                cent = torch.where(keep[:, None], cent, new)
            items, offsets = assign(cent)
            sizes = (offsets[1:] - offsets[:-1]).tolist()
            self.ivf = SimpleNamespace(n_lists=L, iters=iters, seed=seed, centroids=cent, list_offsets=offsets, list_items=items,
                                       pooled_sorted=x[items.long()].contiguous(), sizes=sizes, sizes_desc=sorted(sizes, reverse=True))
        return self

    def _check_nprobe(self, nprobe, n_candidates=None):
        if nprobe is None:
            return None
        if self.ivf is None:
            raise ValueError(f"nprobe={nprobe!r} needs the gallery's inverted file: call build_ivf(...) first")
        nprobe = check_nprobe(nprobe, self.ivf.n_lists)
        if n_candidates == 0:
            raise ValueError("nprobe restricts the prefilter: the exhaustive path (n_candidates = 0) has none")
        return nprobe

    def ivf_candidates(self, pooled_q, n_candidates, nprobe, chunk=256):
        """(cand [n, C] int32, pool_len [n] int32) of pooled query vectors [n, d]: every query's pool = the members of the nprobe
        lists whose centroids score highest against it (the order of 6.1: score descending, ties by lower list), its candidates
        = the top C of the pool by (coarse score descending, gallery index ascending) in ascending gallery index, -1 where the
        pool holds fewer.  Per pass of queries: ops.gemm_nt_f32 + ops.slab_topk_rows name the probes, ops.ivf_scan scores the
        pool, ops.ivf_select reduces it.  No host read: the buffers are sized by the P largest lists, known since the build."""
        C, chunk = check_candidates(n_candidates), check_chunk(chunk)
        P = self._check_nprobe(nprobe)
        if P is None:
            raise ValueError("ivf_candidates needs nprobe")
        ivf = self.ivf
        n, dev = pooled_q.shape[0], pooled_q.device
        cand = torch.empty((n, C), dtype=torch.int32, device=dev)
        pool_len = torch.empty((n,), dtype=torch.int32, device=dev)
        if n == 0:
            return cand, pool_len
        stride = max(sum(ivf.sizes_desc[:P]), 1)
        # a pass takes as many queries as fit the memory of the exact prefilter's [chunk, N] block: its two pool buffers are
        # [rows, stride] of 4 bytes each, so rows = chunk N / (2 stride) >= chunk -- fewer, larger launches (the lists do not
        # depend on the split)
        chunk = max(chunk, chunk * len(self) // (2 * stride))
        rows = min(chunk, n)
        score = torch.empty((rows, stride), dtype=torch.float32, device=dev)
        item = torch.empty((rows, stride), dtype=torch.int32, device=dev)
        for lo in range(0, n, chunk):
            pq = pooled_q[lo:lo + chunk].contiguous()
            m = pq.shape[0]
            probes, _ = ops.slab_topk_rows(ops.gemm_nt_f32(pq, ivf.centroids), P)
            pool = ops.ivf_scan(pq, ivf.pooled_sorted, ivf.list_items, ivf.list_offsets, probes, stride, ivf.sizes_desc[0],
                                out=(score[:m], item[:m], pool_len[lo:lo + m]))
            cand[lo:lo + m] = ops.ivf_select(*pool, C)
        return cand, pool_len

    def _check_correction(self, norm, local_scaling, n_candidates, allow_zero=True, mutual_proximity=None):
        """The correction the arguments ask for -> (CandCorrection, mode), or None without one.  Refuses an unknown mode, two
        corrections at once, one that is not attached, the exhaustive path and fewer candidates than the correction works on."""
        modes = check_corrections(norm, local_scaling, mutual_proximity)
        asked = [(c, mode) for c, mode in zip((_NORM, _LOCAL_SCALING, _MUTUAL_PROXIMITY), modes) if mode is not None]
        if not asked:
            return None
        c, mode = asked[0]
        if getattr(self, c.needs) is None:
            raise ValueError(c.missing.format(mode=mode))
        C = check_candidates(n_candidates, allow_zero)      # `candidates` has no exhaustive path: 0 is out of its range
        if C == 0:
            raise ValueError(f"{c.name} acts on candidate lists: the exhaustive path (n_candidates = 0) has the evaluator's corrections")
        if C < c.min_candidates(self):
            raise ValueError(c.too_few.format(need=c.min_candidates(self), C=C))
        return c, mode

    def _check_queries(self, q_feat, q_mask):
        _check_tokens(q_feat, q_mask, "query")
        if q_feat.shape[2] != self.items.d:
            raise ValueError(f"queries are {q_feat.shape[2]} wide, the gallery {self.items.d}")
        if q_feat.device != self.feat.device:
            raise ValueError("queries and gallery must be on the same device")

    def coarse_scores(self, pooled_q):
        """[n_q, N] fp32 cosines of pooled query vectors against the gallery's (nr_gemm_nt_f32: exact fp32 products, one
        fixed summation order per element)."""
        return ops.gemm_nt_f32(pooled_q, self.items.pooled)

    def candidates(self, q_feat, q_mask, n_candidates, chunk=256, norm=None, nprobe=None, ivf_stats=False, local_scaling=None,
                   mutual_proximity=None):
        """(cand [n, C] int32, fine [n, C] fp32): every query's C candidates in ascending gallery index (padded with -1 when
        the gallery has fewer than C items) and their fine scores (-inf at the padding).  norm "is" | "qbnorm" (after
        attach_querybank): (cand, fine, corr [n, C] fp32, gate [n] int32), the corrected scores and which queries were normalised
        ("is": all of them; "qbnorm": those whose top-1 candidate is in the activation set).

        nprobe = P (after build_ivf; 1 <= P <= min(L, 128)): the candidates come from the query's P probed lists only (DESIGN.md
        6.16); None is the exact prefilter.  ivf_stats (with nprobe): one more result, stats [n, 3] int32 = (the pool's length,
        how many of the exact prefilter's candidates the list kept, how many candidates the exact prefilter has): the exact
        lists are computed for these counts only.

        local_scaling "csls" | "nicdm" | "ls" (after attach_localscale; not with norm; n_candidates >= ls_k): (cand, fine, corr
        [n, C] fp32, qstat [n, 2] fp32), the locally scaled scores and every query's own (mean, kth) of the top
        ls_k of its candidates' fine scores.

        mutual_proximity "emp" | "gauss" (after attach_mutualprox; not with norm or local_scaling): (cand, fine, corr [n, C] fp32,
        qstat [n, 3] fp32), the mutual-proximity scores and every query's own (count, mean, sd) of its
        candidates' fine scores."""
        correction = self._check_correction(norm, local_scaling, n_candidates, allow_zero=False, mutual_proximity=mutual_proximity)
        nprobe = self._check_nprobe(nprobe)
        if ivf_stats and nprobe is None:
            raise ValueError("ivf_stats describes the inverted-file prefilter: it needs nprobe")
        if correction is not None:
            return self._corrected(q_feat, q_mask, 1, n_candidates, chunk, correction, nprobe, ivf_stats)[2:]
        C, chunk = check_candidates(n_candidates), check_chunk(chunk)
        self._check_queries(q_feat, q_mask)
        dev = q_feat.device
        n = q_feat.shape[0]
        if n == 0:
            empty = (torch.empty((n, C), dtype=torch.int32, device=dev), torch.empty((n, C), dtype=torch.float32, device=dev))
            return empty + ((torch.empty((0, 3), dtype=torch.int32, device=dev),) if ivf_stats else ())
        with torch.no_grad():
            q = _Side(self.model, q_feat, q_mask, self.query_side)
            cand, pool_len, exact = self._prefilter(q.pooled, C, chunk, nprobe, ivf_stats)
            g = self.items
            fine = ops.local_level_cand(q.prep, g.prep, q.w, g.w, n, q.n_tok, g.n, g.n_tok, cand, hip.PREC_BF16X3)
            if ivf_stats:
                kept = torch.empty_like(pool_len)
                for lo in range(0, n, chunk):                           # [chunk, C, C] comparisons at a time
                    e = exact[lo:lo + chunk]
                    kept[lo:lo + chunk] = ((e[:, :, None] == cand[lo:lo + chunk, None, :]) & (e[:, :, None] >= 0)).any(dim=2).sum(dim=1)
                return cand, fine, torch.stack([pool_len, kept, (exact >= 0).sum(dim=1).to(torch.int32)], dim=1)
        return cand, fine

    def _prefilter(self, pooled_q, C, chunk, nprobe=None, want_exact=False):
        """The coarse stage for pooled query vectors [n, d], n >= 1 -> (cand [n, C] int32, pool_len [n] int32 or None, exact).
        nprobe None: the exact prefilter (cand is exact).  nprobe = P: the inverted file's candidates and pool lengths; exact =
        the exact prefilter's lists when want_exact, else None."""
        n = pooled_q.shape[0]
        exact = None
        if nprobe is None or want_exact:
            exact = torch.empty((n, C), dtype=torch.int32, device=pooled_q.device)
            big = torch.iinfo(torch.int32).max
            for lo in range(0, n, chunk):
                ci, _ = ops.slab_topk_rows(self.coarse_scores(pooled_q[lo:lo + chunk].contiguous()), C)
                ci = torch.where(ci < 0, torch.full_like(ci, big), ci).sort(dim=1).values       # ascending index, padding last
                exact[lo:lo + chunk] = torch.where(ci == big, torch.full_like(ci, -1), ci)
        if nprobe is None:
            return exact, None, exact
        return self.ivf_candidates(pooled_q, C, nprobe, chunk) + (exact,)

    def _corrected(self, q_feat, q_mask, k, n_candidates, chunk, correction, nprobe=None, ivf_stats=False):
        """(idx, val, cand, fine, corr, extra[, stats]): the candidates and their fine scores, then the correction's one launch
        (extra: gate of norm, qstat of local_scaling and of mutual_proximity)."""
        c, mode = correction
        cand, fine, *stats = self.candidates(q_feat, q_mask, n_candidates, chunk, nprobe=nprobe, ivf_stats=ivf_stats)
        idx, val, corr, extra = c.rerank(self, mode, fine, cand, k)
        return (idx, val, cand, fine, corr, extra) + tuple(stats)

    def search(self, q_feat, q_mask, k, n_candidates, chunk=256, return_candidates=False, norm=None, nprobe=None, local_scaling=None,
               mutual_proximity=None):
        """-> (idx [n, k] int32, val [n, k] fp32): the top k of every query, fine score descending, ties by lower gallery index,
        padded with -1 / -inf when the gallery has fewer than k items.  1 <= k <= n_candidates <= 128; n_candidates = 0 scores
        every pair (the exhaustive path: the evaluator's slab similarity and ops.slab_topk_rows).  return_candidates: also the
        candidate lists and their fine scores, (idx, val, cand, fine).  norm "is" | "qbnorm" (after attach_querybank): the
        order and val are those of the corrected scores; with return_candidates (idx, val, cand, fine, gate).  nprobe = P (after
        build_ivf): the candidates come from the P probed lists of the inverted file; not with n_candidates = 0.
        local_scaling "csls" | "nicdm" | "ls" (after attach_localscale; not with norm, n_candidates >= ls_k): the order and val are
        those of the locally scaled scores; with return_candidates (idx, val, cand, fine, qstat).
        mutual_proximity "emp" | "gauss" (after attach_mutualprox; not with norm or local_scaling): the order and val are those of
        the mutual-proximity scores; with return_candidates (idx, val, cand, fine, qstat [n, 3])."""
        C, chunk = check_candidates(n_candidates, allow_zero=True), check_chunk(chunk)
        if not _int_in(k, 1, C or hip.TOPK_MAX):
            raise ValueError(f"k must be an integer in [1, {C or hip.TOPK_MAX}] (1 <= k <= n_candidates), got {k!r}")
        correction = self._check_correction(norm, local_scaling, C, mutual_proximity=mutual_proximity)
        nprobe = self._check_nprobe(nprobe, C)
        self._check_queries(q_feat, q_mask)
        if correction is not None:
            idx, val, cand, fine, _, extra = self._corrected(q_feat, q_mask, k, C, chunk, correction, nprobe)
            return (idx, val, cand, fine, extra) if return_candidates else (idx, val)
        if C == 0:
            if return_candidates:
                raise ValueError("the exhaustive path (n_candidates = 0) has no candidate lists")
            return self._exhaustive(q_feat, q_mask, k, chunk)
        cand, fine = self.candidates(q_feat, q_mask, C, chunk, nprobe=nprobe)
        idx, val = rerank(cand, fine, k)
        return (idx, val, cand, fine) if return_candidates else (idx, val)

    def _exhaustive(self, q_feat, q_mask, k, chunk):
        from .evaluator import _slab_similarity
        n = q_feat.shape[0]
        if self.side == "video":
            S = _slab_similarity(self.model, q_feat, self.feat, q_mask, self.mask, 0, n, chunk)
        else:
            S = _slab_similarity(self.model, self.feat, q_feat, self.mask, q_mask, 0, len(self), chunk).T.contiguous()
        if n == 0:
            return (torch.empty((0, k), dtype=torch.int32, device=S.device), torch.empty((0, k), dtype=torch.float32, device=S.device))
        return ops.slab_topk_rows(S, k)


def rerank(cand, fine, k):
    """The top k of candidate lists in ascending index order: (idx [n, k] int32, val [n, k] fp32), fine score descending, ties by
    lower position = lower gallery index; absent slots -1 / -inf."""
    n = cand.shape[0]
    if n == 0:
        return (torch.empty((0, k), dtype=torch.int32, device=cand.device), torch.empty((0, k), dtype=torch.float32, device=cand.device))
    pos, val = ops.slab_topk_rows(fine, k)
    idx = torch.gather(cand, 1, pos.clamp(min=0).long())
    gone = (pos < 0) | (idx < 0)
    idx = torch.where(gone, torch.full_like(idx, -1), idx)
    val = torch.where(gone, torch.full_like(val, float("-inf")), val)
    return idx, val
