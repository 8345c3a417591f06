"""fp64 restatement of the row-loss tail, ROW BY ROW (until_module.py:56-359; the kernels: csrc/nr_rowloss.hip, the uniform
rows of csrc/nr_sinkhorn.hip, csrc/nr_finalize.h, nr_rowloss_coef / nr_rowloss_bwd_finish).  Plain torch on the CPU; nothing
here calls the library.  What tests/slab_terms_torch.py and oracle/nr_oracle.py sum over the batch is kept apart here:

  row_terms(...) -> [2, 4, B]     rowloss[dir][term][i], terms = centrality, uniform, neighbour, KL; direction 1 is the same
                                  function on S.t(), G.t(), tgt_cols, c1, w_v (the reference's "v2t" call)
  five_losses, centres_from_parts, centrality_weights, coef, grads: the arithmetic around it, see each function.

Every function takes `dtype`: float64 is the reference, float32 the TWIN -- the same formulas in plain fp32 on the same inputs.
The twin's distance from the reference is what the arithmetic itself costs in fp32; the GPU tests' bars are FACTOR times that
(E32_* / BAR_* below), never anything measured on a kernel.  tests/test_rowloss_cpu.py recomputes every E32 on the inputs of
every GPU case (the case lists below) and holds the stored bars to them.

Inputs (make_case): S = a 2^-12 grid in [-0.3, 0.3] (negative similarities included) + a Latin-square offset of 2^-24 steps, so
no two entries of a row or of a column are equal BY CONSTRUCTION (the top-K sets of kernel and reference are then the same
sets, whatever the rounding), + a diagonal bump; G = 6 randn + 8 I; c = 0.05 randn (both signs); w = exp(0.05 randn);
logit scale 100; T = 3; targets = 0.7 softmax(2 randn) + 0.3 I (any non-negative rows do: no Sinkhorn solve involved)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from slab_terms_torch import neighbor_rows

TERMS = ("centrality", "uniform", "neighbour", "kl")
GRADS = ("dS", "dG", "d_c0", "d_c1", "d_w_t", "d_w_v", "d_ls")

# ---- tolerances ---------------------------------------------------------------------------------------------------------------
# E32_*: max over the case lists below of  max|twin - fp64| / max|fp64|  (per case, then the largest), measured on the CPU
# by tests/test_rowloss_cpu.py (which recomputes them and fails if a bar below is less than FACTOR times its value, or above
# its cap).  FACTOR covers what the twin does not model: a 64-lane tree sum instead of torch's order, expf / logf at up to
# 2 ulp, 1 / (max - min) as a reciprocal.  Bars are RELATIVE to max|reference| of the term (gradient) in the case at hand.
FACTOR = 8.0
# measured 9.81e-8 / 2.37e-7 / 4.23e-7 / 3.93e-7 (the same with 1, 4 and 16 CPU threads), stored with a tenth of headroom
E32_FWD = {"centrality": 1.1e-7, "uniform": 2.6e-7, "neighbour": 4.7e-7, "kl": 4.4e-7}
BAR_FWD = {k: FACTOR * v for k, v in E32_FWD.items()}          # 8.8e-7 / 2.1e-6 / 3.8e-6 / 3.5e-6
CAP_FWD = 1e-4                                       # the bar tests/test_kernels_gpu.py::test_row_losses uses on batch means
# measured 2.85e-7 / 1.06e-6 / 2.15e-5 / 9.89e-5 / 1.23e-7 / 1.19e-7 / 1.12e-7.  d_c0 / d_c1 are column sums over all rows of
# terms that cancel (the neighbour term does not change when c is shifted): the twin itself loses that much at B = 513 / 1025.
E32_BWD = {"dS": 3.2e-7, "dG": 1.2e-6, "d_c0": 2.4e-5, "d_c1": 1.1e-4, "d_w_t": 1.4e-7, "d_w_v": 1.4e-7, "d_ls": 1.3e-7}
BAR_BWD = {k: FACTOR * v for k, v in E32_BWD.items()}          # 2.6e-6 / 9.6e-6 / 1.9e-4 / 8.8e-4 / 1.1e-6 / 1.1e-6 / 1.0e-6
CAP_BWD = 1e-3                                       # test_neighbour_term_gradient_matches_oracle_autograd's
BAR_SINKHORN_UNIFORM = 2e-5                          # nr_sinkhorn.hip's uniform rows (__expf / __logf / rcp, matrix scaling:
#                                                      not modelled by the twin): the suite's bar for that launch, kept
BAR_COEF = 1e-6

# ---- the GPU cases (tests/test_rowloss_gpu.py runs exactly these; tests/test_rowloss_cpu.py measures the twin on them) --------
# nr_row_ne switches at B = 128 / 256 / 512 / 1024, valid[e] at multiples of 64, the last workgroup is partial when B % 4 != 0.
# (3, 1) has K = B - 2: ONE sample outside the neighbour set, min = max there and the reference's neighbour rows are NaN
# (until_module.py:85, 0 / 0) -- compared as NaN positions, like the constant-c case.
# B = 129 / 257 / 513 / 1025 enter the NE = 4 / 8 / 16 / 32 instances with ONE valid entry in their first new register;
# 256 / 512 / 1024 (and 2048) fill every register of an instance.
FWD_CASES = [(2, 1, ""), (3, 1, "nan"), (5, 2, ""), (64, 20, ""), (65, 20, ""), (127, 20, ""), (129, 20, ""), (257, 20, ""),
             (513, 20, ""), (1025, 20, ""), (2048, 20, ""), (256, 20, ""), (512, 20, ""), (1024, 20, ""),
             (9, 0, ""), (13, 12, ""), (13, 13, ""), (70, 20, "ties"), (12, 3, "const_c")]
SLABS = [(70, 0, 70), (70, 33, 5), (129, 128, 1), (257, 60, 130)]                       # (B, row0, n); K = 20
PARTS_B = [(4, 1), (36, 20), (128, 20)]                                                 # (B, K)
PARTS_N = [(1, 1), (3, 4), (5, 16), (7, 2)]                                             # (n_c0, n_c1)
PARTS_SCALE = [1.0 / 512, 1.0 / 7]
CW_B = [(4, 1), (100, 20)]
CW_D = [4, 260, 512, 768]
CW_SCALE = 0.3
BWD_CASES = [(5, 2), (33, 8), (65, 20), (129, 20), (257, 20), (513, 20), (1025, 20), (13, 12), (13, 13)]
# upstream gradients of (total, centrality, uniform, neighbour, kl) and the three weights
UPSTREAM = [((1.7, None, None, None, None), (0.5, 2.0, 1.5)),
            ((None, 0.9, -1.3, 2.1, 0.6), (0.5, 2.0, 1.5))]
SINKHORN_B = [4, 8, 20, 36, 64, 100, 124, 128]
SINKHORN_BETA = [0.7, 1.0, 0.0]
# The Sinkhorn cases add one too: max|reference uniform term| >= 1 in every case.  With seed 4246 all four rows of B = 4 are
# dominated by their diagonal, the term is what is left of T x_ii - LSE(T x) (two numbers near 40) at 1e-5 .. 0.06, and the
# fp32 twin is 2e-3 of it away: one ulp of the operands, whatever evaluates them.
SEED_FWD, SEED_PARTS, SEED_CW, SEED_SINKHORN = 4242, 4243, 4244, 4247
# The backward cases add a condition on the inputs (asserted in tests/test_rowloss_cpu.py): in every row the rest set's range
# of c and of S is at least MIN_REST_RANGE.  d_c carries 1 / (max - min) of c over the rest set; with the 2 samples a rest set
# has at B = 5 a range of 0.004 (seed 4245) puts the fp32 TWIN 4e-4 away from fp64 -- no fp32 kernel can be held to that input.
SEED_BWD = 4250
MIN_REST_RANGE = 0.01


def sinkhorn_iters(B):
    return (0, 1, 2, 50) if B in (20, 128) else (50,)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _direction(S, G, tgt, c, w, ls, K, T):
    B = S.shape[0]
    d = torch.arange(B)
    cent = -torch.log_softmax(S * ls, dim=-1)[d, d] * w                                 # until_module.py:315-327
    unif = -(torch.log_softmax(G * T, dim=-1) * tgt).sum(-1)                             # :285-289
    lp = torch.log_softmax(S, dim=-1)
    kl = (lp.exp() * (lp - torch.log_softmax(G, dim=-1))).sum(-1)                        # :351-357
    neigh = neighbor_rows(S, c, K, T, d)                                                 # :161-211
    return torch.stack((cent, unif, neigh, kl))


def row_terms(S, G, tgt_rows, tgt_cols, c0, c1, w_t, w_v, ls, K, T, dtype=torch.float64):
    """-> [2, 4, B] in `dtype`.  ls: python float or a one-element tensor."""
    f = lambda t: t.to(dtype)
    S, G = f(S), f(G)
    ls = f(ls.reshape(())) if torch.is_tensor(ls) else ls
    return torch.stack((_direction(S, G, f(tgt_rows), f(c0), f(w_t), ls, K, T),
                        _direction(S.t(), G.t(), f(tgt_cols), f(c1), f(w_v), ls, K, T)))


def case_terms(q, dtype=torch.float64, **over):
    """row_terms of a make_case() namespace; `over` replaces single inputs (c0=..., w_t=...)."""
    a = dict(S=q.S, G=q.G, tgt_rows=q.tgt_rows, tgt_cols=q.tgt_cols, c0=q.c0, c1=q.c1, w_t=q.w_t, w_v=q.w_v, ls=q.ls)
    a.update(over)
    with torch.no_grad():
        return row_terms(a["S"], a["G"], a["tgt_rows"], a["tgt_cols"], a["c0"], a["c1"], a["w_t"], a["w_v"], a["ls"], q.K, q.T, dtype)


def uniform_rows(G, tgt_rows, tgt_cols, T, dtype=torch.float64):
    """Term 1 alone -> [2, B]: -sum_j tgt[i, j] * log_softmax(T * X)[i, j], X = G / G.t()  (until_module.py:285-289)."""
    G = G.to(dtype)
    return torch.stack((-(torch.log_softmax(G * T, dim=-1) * tgt_rows.to(dtype)).sum(-1),
                        -(torch.log_softmax(G.t() * T, dim=-1) * tgt_cols.to(dtype)).sum(-1)))


def five_losses(rows, wu, wn, wkl):
    """(total, centrality, uniform, neighbour, kl) from rows [2, 4, B]: the arithmetic of nr_finalize.h (modeling.py:329-358; the
    kl term is divided by B once more: kl_div 'mean' divides by B * B) in the dtype of `rows`."""
    B = rows.shape[-1]
    m = rows.sum(-1) / B                                       # [2, 4]
    c, u, n = ((m[0, k] + m[1, k]) / 2 for k in range(3))
    k = (m[0, 3] / B + m[1, 3] / B) / 2
    return torch.stack((c + u * wu + n * wn + k * wkl, c, u, n, k))


def centres_from_parts(parts, scale, dtype=torch.float64):
    """c_j = scale * sum_p parts[p][j]  (until_module.py:181 on the partial sums of the bank products)."""
    return parts.to(dtype).sum(0) * scale


def centrality_weights(g, mean, scale, dtype=torch.float64):
    """exp(scale * <g_i, mean> / max(|g_i|, 1e-12))  (modeling.py:403-430, one global token per sample); g [B, d], mean [d]."""
    g, mean = g.to(dtype), mean.to(dtype)
    return torch.exp(scale * (g @ mean) / g.norm(dim=-1).clamp_min(1e-12))


def coef(g5, wu, wn, wkl, B, dtype=torch.float64):
    """g_rowloss [2, 4, B] from the gradients of the five losses (floats or None): five_losses differentiated --
    coef[term] = (g_total * weight[term] + g_term) * 0.5 / B, the kl term divided by B once more."""
    t = 0.0 if g5[0] is None else g5[0]
    g = [0.0 if x is None else x for x in g5[1:]]
    h = 0.5 / B
    c = torch.tensor([(t + g[0]) * h, (t * wu + g[1]) * h, (t * wn + g[2]) * h, (t * wkl + g[3]) / B * h], dtype=dtype)
    return c[None, :, None].expand(2, 4, B).contiguous()


def grads(q, g_rowloss, dtype=torch.float64):
    """Autograd of sum(g_rowloss * row_terms(...)) in `dtype`, the targets constant.
    -> dict(dS, dG, d_c0, d_c1, d_w_t, d_w_v, d_ls)."""
    leaves = [t.to(dtype).clone().requires_grad_() for t in (q.S, q.G, q.c0, q.c1, q.w_t, q.w_v, q.ls)]
    S, G, c0, c1, w_t, w_v, ls = leaves
    rows = row_terms(S, G, q.tgt_rows, q.tgt_cols, c0, c1, w_t, w_v, ls, q.K, q.T, dtype)
    (g_rowloss.to(dtype) * rows).sum().backward()
    out = dict(zip(GRADS, (t.grad for t in leaves)))
    out["d_ls"] = out["d_ls"].reshape(())
    return out


def neighbor_rows_loop(S, c, K, T):
    """The neighbour term (until_module.py:161-211) one row at a time in Python doubles: for tiny problems only.  S [B, B],
    c [B] -> list of B floats.  Ties in the top-K go to the lower column."""
    S, c = S.double().tolist(), c.double().tolist()
    B = len(S)
    out = []
    for i in range(B):
        order = sorted((j for j in range(B)), key=lambda j: (-(S[i][j] if j != i else -9e15), j))
        nb = order[:K]
        ext = set(nb) | {i}
        rest = [j for j in range(B) if j not in ext]
        lo_s, hi_s = (min(S[i][j] for j in rest), max(S[i][j] for j in rest)) if rest else (9e15, -9e15)
        lo_c, hi_c = (min(c[j] for j in rest), max(c[j] for j in rest)) if rest else (9e15, -9e15)
        adj = {j: T * ((S[i][j] - lo_s) / (hi_s - lo_s) - (c[j] - lo_c) / (hi_c - lo_c)) for j in nb}
        p = {}
        if nb:
            m = max(adj.values())
            tot = math.fsum(math.exp(a - m) for a in adj.values())
            p = {j: math.exp(adj[j] - m) / tot for j in nb}
        p[i] = 1.0                                             # fill_diagonal_(1), also when the diagonal is a "neighbour" (K = B)
        m = max(S[i][j] for j in ext)
        lse = m + math.log(math.fsum(math.exp(S[i][j] - m) for j in ext))
        out.append(-math.fsum(p[j] * (S[i][j] - lse) for j in ext) / math.fsum(p.values()))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def make_S(seed, B, ties=False):
    """fp32 [B, B] in about [-0.3, 0.3] + 80 / 4096 on the diagonal.  ties=False: grid of 2^-12 plus ((5 i + 3 j) mod 2048) 2^-24,
    exact in fp32 and distinct along every row and every column (B <= 2048).  ties=True: a grid of 1/32 alone -- about 20
    levels, so exact ties everywhere, across the top-K boundary of most rows too."""
    from neighborretr_amd import synth
    assert B <= 2048
    u = synth.uniform(seed, "rowloss/S", (B, B))
    if ties:
        S = np.round((u - 0.5) * 0.6 * 32) / 32
    else:
        i, j = np.arange(B)[:, None], np.arange(B)[None, :]
        S = np.round((u - 0.5) * 0.6 * 4096) / 4096 + ((5 * i + 3 * j) % 2048) * 2.0 ** -24
    S = S + np.eye(B) * (80.0 / 4096)
    out = _t(S)
    assert np.array_equal(out.numpy().astype(np.float64), S)          # exactly representable
    return out


def make_G(seed, B, sigma=6.0, diag=8.0):
    from neighborretr_amd import synth
    return _t(sigma * synth.normal(seed, "rowloss/G", (B, B)) + diag * np.eye(B))


def make_case(seed, B, K, ties=False, const_c=False):
    """The inputs of one row-kernel case, fp32 CPU tensors in a namespace (see the module docstring)."""
    from neighborretr_amd import synth
    q = SimpleNamespace(B=B, K=K, T=3.0)
    q.S = make_S(seed, B, ties)
    q.G = make_G(seed, B)
    for name in ("c0", "c1"):
        c = 0.05 * synth.normal(seed, "rowloss/" + name, (B,))
        setattr(q, name, _t(np.full(B, 0.05) if const_c else c))
    q.w_t = _t(np.exp(0.05 * synth.normal(seed, "rowloss/w_t", (B,))))
    q.w_v = _t(np.exp(0.05 * synth.normal(seed, "rowloss/w_v", (B,))))
    q.ls = torch.tensor([100.0])
    for name in ("tgt_rows", "tgt_cols"):
        z = torch.from_numpy(2.0 * synth.normal(seed, "rowloss/" + name, (B, B)))
        setattr(q, name, (0.7 * torch.softmax(z, dim=-1) + 0.3 * torch.eye(B, dtype=torch.float64)).float().contiguous())
    return q


def make_parts(seed, B, n, scale, name):
    """[n, B] fp32 partial sums of both signs whose scaled sum is about 0.05 randn."""
    from neighborretr_amd import synth
    return _t(synth.normal(seed, f"rowloss/parts/{name}/{n}", (n, B)) * (0.05 / (scale * math.sqrt(n))))


def make_cw(seed, B, d):
    """(g_text, g_video [B, d], mean_text, mean_video [d]): randn tokens with row 1 of both all zeros (the max(., 1e-12) branch:
    weight exactly 1), two DIFFERENT means of 0.5 randn."""
    from neighborretr_amd import synth
    g_t, g_v = (synth.normal(seed, f"rowloss/cw/g_{s}/{d}", (B, d)) for s in "tv")
    g_t[1] = 0.0
    g_v[1] = 0.0
    m_t, m_v = (0.5 * synth.normal(seed, f"rowloss/cw/mean_{s}/{d}", (d,)) for s in "tv")
    return _t(g_t), _t(g_v), _t(m_t), _t(m_v)


def rest_sets(S, K):
    """bool [B, B]: the rest set of every row (neither diagonal nor one of the K neighbours; ties -> lower column)."""
    B = S.shape[0]
    eye = torch.eye(B, dtype=torch.bool)
    s = torch.where(eye, torch.full_like(S, -9e15), S)
    idx = torch.sort(s, dim=-1, descending=True, stable=True)[1][:, :K]
    return ~(torch.zeros_like(eye).scatter_(1, idx, True) | eye)


def rel_err(got, want):
    """max|got - want| / max|want| in fp64 (0 when both are all zero); NaN if either side holds a NaN."""
    got, want = got.detach().double(), want.detach().double()
    den = float(want.abs().max())
    num = float((got - want).abs().max())
    return num / den if den > 0 else num
