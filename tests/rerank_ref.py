"""fp64 restatements of two-stage retrieval (neighborretr_amd/search.py, evaluator.two_stage_evaluation), written
with plain loops and NumPy so that the tests do not compare the code under test with itself.

  pair_scores / similarity   the fine score 0.5 (sum_t w_q max_v + sum_v w_g max_t) of chosen pairs / of every pair
  pooled / coarse            p(x) = normalize(sum_tok w[tok] x^[tok]) and the cosines p_q . p_g
  select                     the top C of every coarse row (score descending, ties by lower index), sorted by ascending index
  final_order                the top k of a candidate list by fine score, ties by lower index
  counts / metrics           found / greater / equal per query and the dictionary built from them
  multi_sentence             the same for ragged sentence groups
"""
import numpy as np
import torch

CUTS = (1, 5, 10, 50)


def unit_tokens(x, mask):
    """x^: the normalised, masked tokens in fp64 (F.normalize's eps 1e-12)."""
    x = torch.as_tensor(x).double()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * torch.as_tensor(mask).double()[..., None]


def similarity(q, qm, w_q, g, gm, w_g):
    """S [n_q, n_g] fp64: the fine score of every pair."""
    R = torch.einsum("atd,bvd->abtv", unit_tokens(q, qm), unit_tokens(g, gm))
    w_q, w_g = torch.as_tensor(w_q).double(), torch.as_tensor(w_g).double()
    return 0.5 * ((R.max(-1).values * w_q[:, None, :]).sum(-1) + (R.max(-2).values * w_g[None]).sum(-1))


def pair_scores(S, cand):
    """out[i, c] = S[i, cand[i, c]], -inf where cand[i, c] lies outside [0, n_g)."""
    S, cand = np.asarray(S, dtype=np.float64), np.asarray(cand)
    out = np.full(cand.shape, -np.inf)
    for i in range(cand.shape[0]):
        for c in range(cand.shape[1]):
            if 0 <= cand[i, c] < S.shape[1]:
                out[i, c] = S[i, cand[i, c]]
    return out


def pooled(x, mask, w):
    """p [n, d] fp64; a fully masked item gives the zero vector."""
    u = (unit_tokens(x, mask) * torch.as_tensor(w).double()[..., None]).sum(1)
    return u / u.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def coarse(p_q, p_g):
    return (p_q @ p_g.T).numpy()


def select(scores, C):
    """cand [n, C] int32: per row the C best columns (score descending, ties by lower index), then in ascending index; -1 pads a
    row of fewer than C columns."""
    scores = np.asarray(scores)
    out = np.full((scores.shape[0], C), -1, dtype=np.int32)
    for i, row in enumerate(scores):
        best = sorted(range(len(row)), key=lambda j: (-row[j], j))[:C]
        out[i, :len(best)] = sorted(best)
    return out


def final_order(cand, fine, k):
    """(idx [n, k] int32, val [n, k]): per list the k best valid candidates, fine score descending, ties by lower gallery index;
    -1 / -inf pad."""
    cand, fine = np.asarray(cand), np.asarray(fine)
    idx = np.full((cand.shape[0], k), -1, dtype=np.int32)
    val = np.full((cand.shape[0], k), -np.inf, dtype=fine.dtype)
    for i in range(cand.shape[0]):
        valid = [c for c in range(cand.shape[1]) if cand[i, c] >= 0]
        best = sorted(valid, key=lambda c: (-fine[i, c], cand[i, c]))[:k]
        for s, c in enumerate(best):
            idx[i, s], val[i, s] = cand[i, c], fine[i, c]
    return idx, val


def counts(cand, fine, gt):
    """[(found, greater, equal)] per query: gt[i] among the candidates, the candidates scoring above it, those equal to it (itself
    included)."""
    out = []
    for i in range(len(cand)):
        own = [fine[i][c] for c in range(len(cand[i])) if cand[i][c] == gt[i]]
        if not own:
            out.append((False, 0, 0))
            continue
        valid = [fine[i][c] for c in range(len(cand[i])) if cand[i][c] >= 0]
        out.append((True, sum(1 for s in valid if s > own[0]), sum(1 for s in valid if s == own[0])))
    return out


def metrics(cnt, C):
    """The dictionary of one direction: a found query contributes the ranks greater .. greater + equal - 1, a missed one a single
    entry that fails at every K."""
    ind = [g + e for f, g, eq in cnt if f for e in range(eq)]
    missed = sum(1 for f, _, _ in cnt if not f)
    total = len(ind) + missed
    m = {f"R{K}": (sum(1 for r in ind if r < K) * 100.0 / total if K <= C else None) for K in CUTS}
    m["cand_recall"] = (len(cnt) - missed) * 100.0 / len(cnt)
    m["n_candidates"] = C
    m["cols"] = ind
    if missed == 0:
        m["MR"] = m["MedianR"] = float(np.median(ind)) + 1
        m["MeanR"] = float(np.mean(ind)) + 1
    return m


def single_sentence(cand_t, fine_t, cand_v, fine_v, C):
    n = len(cand_t)
    return metrics(counts(cand_t, fine_t, range(n)), C), metrics(counts(cand_v, fine_v, range(n)), C)


def multi_sentence(cand_t, fine_t, cand_v, fine_v, ends, C):
    """(t2v, v2t) for sentence groups; ends[g] = one past the last sentence of video g."""
    group = [next(g for g, e in enumerate(ends) if s < e) for s in range(len(cand_t))]
    ranks, missed = [], 0
    for s in range(len(cand_t)):
        own = [fine_t[s][c] for c in range(len(cand_t[s])) if cand_t[s][c] == group[s]]
        if not own:
            missed += 1
            continue
        ranks.append(sum(1 for c in range(len(cand_t[s])) if cand_t[s][c] >= 0 and (
            fine_t[s][c] > own[0] or (fine_t[s][c] == own[0] and cand_t[s][c] < group[s]))))
    Ns = len(cand_t)
    t2v = {f"R{K}": (sum(1 for r in ranks if r < K) * 100.0 / Ns if K <= C else None) for K in CUTS}
    t2v.update(cand_recall=(Ns - missed) * 100.0 / Ns, n_candidates=C, cols=ranks)
    if missed == 0:
        r1 = np.asarray(ranks) + 1
        t2v["MedianR"] = t2v["MR"] = float(np.sort(r1)[(len(r1) - 1) // 2])
        t2v["MeanR"], t2v["Std_Rank"] = float(np.mean(r1)), float(np.std(r1))
    cnt = []
    for j in range(len(cand_v)):
        best = {}
        for c in range(len(cand_v[j])):
            if cand_v[j][c] >= 0:
                g = group[cand_v[j][c]]
                best[g] = max(best.get(g, -np.inf), fine_v[j][c])
        if j not in best:
            cnt.append((False, 0, 0))
        else:
            cnt.append((True, sum(1 for s in best.values() if s > best[j]), sum(1 for s in best.values() if s == best[j])))
    return t2v, metrics(cnt, C)
