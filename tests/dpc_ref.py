"""Decision-exact reference of the DPC-KNN assignment (csrc/nr_cluster.hip: nr_dpc_assign_kernel; csrc/nr_ctm_bodies.h:
nr_ctm_back_body, nr_ctm_back_body2), of the distance matrix it reads and of the cluster shares / means the same wave computes
from it; an fp32 twin of the kernels' arithmetic; the makers of the test inputs and the case lists of tests/test_dpc_cpu.py and
tests/test_dpc_gpu.py.  Plain torch / numpy on the CPU; nothing here calls the library.

WHAT IS COMPARED.  The assignment is a chain of comparisons.  assign_ref takes a distance matrix of fp32 values AS EXACT INPUTS
(on the GPU: the kernel's own matrix, read back from where the kernel left it), evaluates cluster.py:473-507 on it in fp64 with
the build's tie rules -- centre score ties go to the lower index, the nearest centre is the first occurrence of the minimum,
centres join themselves -- and says per sample whether every comparison the result depends on is DECIDED: whether any correct
fp32 evaluation, with or without fused multiply-adds, must come to the same answer.  A kernel is held to equality on decided
samples and only counted on the others.  The masked columns are filled with far = fl32(max over the batch + 1): the one fp32
rounding every fp32 evaluation (the reference's own included) applies there, so that kernels and reference read the same matrix.

COMPARISONS THAT NEED NO MARGIN.  The nearest centre (entries of the matrix against each other), the sample's and the batch's
maximum: raw fp32 entries, compared exactly by everybody.

COMPARISONS THAT DO.  u = 2^-24 (one fp32 rounding, relative).  The kernels compute, per token with its k nearest t_1 <= .. <= t_k
(itself, at 0, included), a = (t_1^2 + .. + t_k^2) / k:
    k squares, summed ascending     every term carries its own rounding and at most k - 1 of the additions: k u on the sum
                                    (fewer with fused multiply-adds)
    one division by (float) k       u                               -> the argument of the exponential is a (1 + (k + 1) u)
    expf                            documented at 1 ulp = 2 u; the argument's error enters as a (k + 1) u relative
    noise * 1e-6f added             the product's rounding is 1e-6 u of the result (counted as u), the addition (or the one
                                    rounding of an fma) u
    density                         (1 + e) exact,  e <= E(k, a) = ((k + 1) a + 4) u
    score = parent * density        parent is a raw entry (exact once the density ORDER is decided): one more u
Two fp32 densities are ordered like the exact ones when the exact ones differ by more than the sum of their error bounds, 2 E.
The pair tolerance is twice that, 4 E: headroom for what the count leaves out (a division or an expf one ulp worse than
documented weighs a u, as much as the whole sum of a small k).
    TOL_DENS  = 64 u        pair tolerance, relative to the larger density: 4 E(k, a) for (k + 1) a <= 12 -- layer-normed tokens
                            at k = 5 have a around 1.6 (distances around sqrt(2), the token itself at 0 among the five)
    TOL_SCORE = 66 u        = TOL_DENS + 2 u (the product, both sides)
Where (k + 1) a is larger (k = N; far-filled columns among the k nearest) the sample's tolerance is 4 max_i E(k, a_i) (+ 2 u for
scores), never less than the constants (assign_ref returns both per sample).  Not tuned against any kernel; tests/test_dpc_cpu.py holds the fp32
twin's measured deviations to 1/8 of them.

A density pair (i, j) is decided when
    * the exact densities differ by more than tol_dens relative to the larger, or
    * both are exactly 0 (masked: the product with the mask's 0), or
    * the two tokens have the SAME exponential term in every evaluation -- bit-identical k-nearest multisets, or sums of squares
      that are exactly representable at every step (dyadic test matrices) and equal -- and either identical noise (then the
      densities are the same bits: neither is denser) or |noise_i - noise_j| * 1e-6 > ulp32(the larger density) + ulp32(the
      larger noise term): rounding is monotone, so the order is the noise's; the two rounded noise terms are still more than
      one ulp of the sum apart, and two numbers more than an ulp apart cannot round together.  (2 ulp32 of the common
      exponential term implies this except across a binade edge; at k = 2 every pair of mutual nearest neighbours is such a
      pair, and the sharper form leaves half as many of them open.)
The centre ranking is decided when, over the first min(cnum + 1, N) scores in sorted order, every neighbouring pair
    * differs by more than tol_score relative, or
    * is 0 and 0 exactly (padding: density 0; duplicates: parent distance 0), or
    * is the same bits: same exponential term, same noise, same parent entry, or
    * has the same parent entry, a power of two (the product is an exact scaling), and a decided density order, or
    * has the same parent entry p and the same exponential term, and p (|noise_i - noise_j| * 1e-6 - ulp32(density) -
      ulp32(noise term)) > ulp32(score): the two fp32 densities are at least that far apart whatever the common term rounds
      to, and products more than an ulp apart do not round together (two runs of repeated frames whose distance is the
      sample's largest: the denser one's parent is the maximum, the other one's the same entry).

dist_ref(xn): fp64 cdist / sqrt(C).  The kernels take C differences (u each, 2 u on the square), square (u), sum the C terms in
some order ((C - 1) u), take a root (half the relative error; the root itself <= 1 ulp = 2 u), multiply by fl32(1 / sqrt(C))
(<= 2 u) with one rounding (u): RIGOROUS relative bound (C / 2 + 6) * 1.01 u for ANY summation order, 0 between identical
rows.  WORKING bar: min(1, 8 * DIST_FRAC[C]) of it, DIST_FRAC[C] = the sequential fp32 twin's measured share
(tests/test_dpc_cpu.py holds the stored figures to what it measures).

merge_ref(xn, w, assign, cnum, proj_b): fp64 shares w / (sum over the cluster + fl32(1e-6)) and cluster means + bias.  Bound
for the kernels' N-term sums: the total of a cluster (N u, any order) + 1e-6 (u), the division (u), the N-term fma chain of
x * share (N u on sum |x| share), the bias (u on the result): merge_bound().  A cluster whose members all have weight 0 (padding)
gives proj_b exactly.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
TOL_DENS = 64 * U
TOL_SCORE = 66 * U
CAP = 0.25                                   # largest share of undecided samples a case may have
FACTOR = 8                                   # working bar = FACTOR x the sequential twin's share of the rigorous bound
E6 = float(np.float32(1e-6))                 # the kernels' 1e-6f
# the sequential fp32 twin's largest |d - ref| / rigorous bound by C, measured 0.1097 / 0.0491 / 0.0369 / 0.0278
DIST_FRAC = {64: 0.12, 256: 0.054, 512: 0.040, 1024: 0.030}
SEED = 4730


def dens_err(k, a):
    """E(k, a): relative error bound of one fp32 density (see above)."""
    return ((k + 1) * a + 4) * U


def _tols(k, a_valid):
    e = dens_err(k, float(a_valid.max())) if a_valid.numel() else 0.0
    return max(TOL_DENS, 4 * e), max(TOL_SCORE, 4 * e + 2 * U)


def far32(dist32):
    """fl32(batch maximum + 1): what fills the masked columns (cluster.py:473-475)."""
    return float(np.float32(np.float32(dist32.max().item()) + np.float32(1.0)))


def masked_matrix(dist32, mask, far=None):
    """The matrix every later step reads, fp64 values that are fp32 numbers."""
    D = dist32.double().clone()
    if mask is not None:
        far = far32(dist32) if far is None else far
        D = torch.where((mask > 0)[:, None, :], D, torch.full_like(D, far))
    return D


def _exact_sums(knn32):
    """Per token: the ascending fp32 sum of squares is exact at every step (then every evaluation order of the kernels gives it)."""
    t = knn32.astype(np.float64)
    ok = np.ones(t.shape[:-1], dtype=bool)
    acc = np.zeros(t.shape[:-1])
    for r in range(t.shape[-1]):
        sq = t[..., r] * t[..., r]
        acc = acc + sq                                       # (fp64: exact for what passes the fp32 tests below)
        ok &= (sq.astype(np.float32).astype(np.float64) == sq) & (acc.astype(np.float32).astype(np.float64) == acc)
    return ok, acc


def assign_ref(dist32, mask, noise32, k, cnum):
    """dist32 [B,N,N] fp32 (exact inputs), mask [B,N] (> 0 = valid) or None, noise32 [B,N] fp32 -> namespace of
    assign [B,N] int64, centres [B,cnum] (rank order), decided [B] bool, density / score [B,N] fp64, tol_dens / tol_score [B],
    a [B,N] (the exponent's argument)."""
    assert dist32.dtype == torch.float32 and noise32.dtype == torch.float32
    B, N, _ = dist32.shape
    D = masked_matrix(dist32, mask)
    valid = (mask > 0) if mask is not None else torch.ones(B, N, dtype=torch.bool)
    knn = torch.sort(D, dim=-1)[0][..., :k]                                   # ascending; ties are equal values
    a = (knn * knn).sum(-1) / k
    dens = torch.exp(-a) + noise32.double() * E6
    dens = dens * valid
    denser = dens[:, None, :] > dens[:, :, None]                              # [b, i, j]: j is denser than i
    dmax = D.flatten(1).max(-1)[0]
    parent = torch.where(denser, D, dmax[:, None, None].expand_as(D)).min(-1)[0]
    score = parent * dens
    order = torch.sort(score, dim=-1, descending=True, stable=True)[1]        # ties -> the lower index
    centres = order[:, :cnum]
    to_c = torch.gather(D, 1, centres[:, :, None].expand(B, cnum, N))
    assign = to_c.argmin(dim=1)                                               # first occurrence
    assign.scatter_(1, centres, torch.arange(cnum)[None, :].expand(B, cnum))  # centres join themselves

    # ---- decided? -----------------------------------------------------------------------------------------------------------
    knn32 = knn.numpy().astype(np.float32)
    exact, acc = _exact_sums(knn32)
    decided = torch.ones(B, dtype=torch.bool)
    tol_d, tol_s = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    nz = noise32.numpy()
    for b in range(B):
        v = valid[b]
        tol_d[b], tol_s[b] = _tols(k, a[b][v])
        d = dens[b].numpy()
        big = np.maximum(d[:, None], d[None, :])
        far_apart = np.abs(d[:, None] - d[None, :]) > tol_d[b].item() * big
        zeros = (d[:, None] == 0) & (d[None, :] == 0)
        same_e = (knn32[b][:, None, :] == knn32[b][None, :, :]).all(-1) | (exact[b][:, None] & exact[b][None, :] & (acc[b][:, None] == acc[b][None, :]))
        dn = np.abs(nz[b][:, None].astype(np.float64) - nz[b][None, :].astype(np.float64))
        ulp = np.spacing(big.astype(np.float32)).astype(np.float64)
        nbig = np.maximum(nz[b][:, None], nz[b][None, :]).astype(np.float64) * E6
        ulp = ulp + np.spacing(nbig.astype(np.float32)).astype(np.float64)
        by_noise = same_e & ((dn == 0) | (dn * E6 > ulp))
        pair_ok = far_apart | zeros | by_noise
        if not pair_ok.all():
            decided[b] = False
            continue
        s, p = score[b].numpy(), parent[b].numpy()
        o = order[b].numpy()
        for r in range(min(cnum + 1, N) - 1):
            i, j = o[r], o[r + 1]
            if abs(s[i] - s[j]) > tol_s[b].item() * max(s[i], s[j]):
                continue
            if s[i] == 0 and s[j] == 0:
                continue
            if p[i] == p[j] and same_e[i, j] and nz[b][i] == nz[b][j]:
                continue
            if p[i] == p[j] and p[i] > 0 and math.frexp(p[i])[0] == 0.5 and d[i] != d[j]:
                continue
            if p[i] == p[j] and same_e[i, j] and p[i] * (dn[i, j] * E6 - ulp[i, j]) > float(np.spacing(np.float32(max(s[i], s[j])))):
                continue
            decided[b] = False
            break
    return SimpleNamespace(assign=assign, centres=centres, decided=decided, density=dens, score=score, parent=parent, a=a,
                           tol_dens=tol_d, tol_score=tol_s)


# ---- the fp32 twin: numpy float32 in the kernels' order of operations, and the planted defects ---------------------------------
DEFECTS = ("scan_ge",          # j > pj -> j >= pj in the k > 4 scan (nr_ctm_back_body2): the scan never leaves its first entry
           "denser_ge",        # > -> >= in the denser-token test
           "ties_high",        # score ties to the higher index
           "nearest_le",       # < -> <= in the nearest-centre loop
           "far_no_plus_1",    # far = the batch maximum, without the + 1
           "dmax_unmasked",    # the sample's maximum taken over unmasked columns only
           "far_sample_max",   # the batch maximum replaced by the sample's
           "no_self_join")     # centres do not join themselves


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def twin32(dist32, mask, noise32, k, cnum, fma=False, defect=None):
    """-> namespace(assign [B,N] int64, density, score [B,N] float32).  fma: the sum of squares and the noise term as fused
    multiply-adds (one rounding), the other way every product is rounded on its own."""
    d_all = dist32.numpy().astype(np.float32)
    B, N, _ = d_all.shape
    nz_all = noise32.numpy().astype(np.float32)
    gmax = d_all.max()
    out = np.zeros((B, N), dtype=np.int64)
    dens_o, score_o = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    for b in range(B):
        D = d_all[b].copy()
        valid = np.ones(N, bool) if mask is None else (mask[b].numpy() > 0)
        if mask is not None:
            top = d_all[b].max() if defect == "far_sample_max" else gmax
            far = top if defect == "far_no_plus_1" else np.float32(top + np.float32(1.0))
            D[:, ~valid] = far
        knn = np.sort(D, axis=1)[:, :k]
        if defect == "scan_ge" and k > 4:
            knn = np.repeat(knn[:, :1], k, axis=1)
        acc = np.zeros(N, np.float32)
        for r in range(k):
            t = knn[:, r]
            if fma:
                acc = _f32(t.astype(np.float64) * t.astype(np.float64) + acc.astype(np.float64))
            else:
                acc = _f32(_f32(t * t) + acc)
        e = np.exp(_f32(-acc / np.float32(k)))
        if fma:
            dens = _f32(nz_all[b].astype(np.float64) * np.float64(np.float32(1e-6)) + e.astype(np.float64))
        else:
            dens = _f32(e + _f32(nz_all[b] * np.float32(1e-6)))
        if mask is not None:
            dens = _f32(dens * valid.astype(np.float32))
        denser = (dens[None, :] >= dens[:, None]) if defect == "denser_ge" else (dens[None, :] > dens[:, None])
        dmax = D[:, valid].max() if (defect == "dmax_unmasked" and valid.any()) else D.max()
        parent = np.minimum(np.where(denser, D, np.float32(np.inf)).min(1), dmax)
        score = _f32(parent * dens)
        idx = np.arange(N)
        order = np.lexsort((-idx if defect == "ties_high" else idx, -score.astype(np.float64)))
        centres = order[:cnum]
        best = np.full(N, np.inf, np.float32)
        bc = np.zeros(N, np.int64)
        for c in range(cnum):
            dv = D[centres[c]]
            take = (dv <= best) if defect == "nearest_le" else (dv < best)
            best = np.where(take, dv, best)
            bc = np.where(take, c, bc)
        if defect != "no_self_join":
            bc[centres] = np.arange(cnum)
        out[b], dens_o[b], score_o[b] = bc, dens, score
    return SimpleNamespace(assign=torch.from_numpy(out), density=dens_o, score=score_o)


# ---- distances -------------------------------------------------------------------------------------------------------------
def dist_rel_bound(C):
    return (C / 2 + 6) * 1.01 * U


def row_ids(x):
    """[B,N] ids, equal where two rows of x [B,N,C] (fp32) are the same bits."""
    B, N, C = x.shape
    return torch.unique(x.contiguous().view(torch.int32).reshape(B * N, C), dim=0, return_inverse=True)[1].view(B, N)


def dist_ref(xn):
    """xn [B,N,C] fp32 -> (fp64 distances [B,N,N], rigorous absolute bound, working absolute bar), entry by entry."""
    C = xn.shape[-1]
    x = xn.double()
    ref = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist") / math.sqrt(C)
    ids = row_ids(xn)
    ref = torch.where(ids[:, :, None] == ids[:, None, :], torch.zeros_like(ref), ref)
    rig = dist_rel_bound(C) * ref
    return ref, rig, min(1.0, FACTOR * DIST_FRAC[C]) * rig


def dist_twin32(xn):
    """The plain loop in fp32: channel after channel, every operation rounded once."""
    x = xn.numpy().astype(np.float32)
    B, N, C = x.shape
    s = np.zeros((B, N, N), np.float32)
    for c in range(C):
        d = x[:, :, None, c] - x[:, None, :, c]
        s = _f32(s + _f32(d * d))
    return torch.from_numpy(_f32(np.sqrt(s) * np.float32(np.float32(1.0) / np.sqrt(np.float32(C)))))


# ---- merge -----------------------------------------------------------------------------------------------------------------
def merge_ref(xn, w, assign, cnum, proj_b):
    """fp64: (shares [B,N], merged + proj_b [B,cnum,C], A = sum |x| share [B,cnum,C], merged [B,cnum,C])."""
    onehot = torch.nn.functional.one_hot(assign, cnum).double()                  # [B,N,c]
    tot = torch.einsum("bnc,bn->bc", onehot, w.double()) + E6
    share = w.double() / torch.gather(tot, 1, assign)
    merged = torch.einsum("bnc,bnd->bcd", onehot, xn.double() * share[..., None])
    A = torch.einsum("bnc,bnd->bcd", onehot, xn.double().abs() * share[..., None])
    return share, merged + proj_b.double(), A, merged


def merge_bound(N, A, merged_pb):
    """Absolute bound of merged_pb, entry by entry (any summation order of the cluster totals)."""
    return 1.01 * U * ((2 * N + 2) * A + merged_pb.abs())


def norm1_ref(merged, w, b, eps):
    return torch.nn.functional.layer_norm(merged, merged.shape[-1:], w.double(), b.double(), eps)


# ---- (a) random inputs -------------------------------------------------------------------------------------------------------
SHAPES = ((3, 1), (4, 1), (8, 3), (9, 3), (12, 3), (24, 4), (32, 4), (33, 5), (64, 11), (64, 16), (24, 24))
KS = (2, 3, 4, 5, "N")


def random_cases():
    """(N, cnum, k, masked) of every random case."""
    out = []
    for N, cnum in SHAPES:
        ks = sorted({N if k == "N" else k for k in KS if k == "N" or k <= N})
        out += [(N, cnum, k, m) for k in ks for m in (False, True)]
    return out


def batch_of(N):
    return 8 if N == 64 else 16


def mask_lengths(B, N, cnum, g):
    """Valid tokens per sample: sample 0 has one, sample 1 two, sample 2 fewer than clusters (where cnum > 1), sample 3 all."""
    ln = torch.randint(1, N + 1, (B,), generator=g)
    ln[0], ln[1], ln[2], ln[3] = 1, min(2, N), max(1, cnum - 1), N
    return ln


def edge_samples(cnum):
    return (0, 1, 2, 3) if cnum > 1 else (0, 1, 3)


# seeds of the random inputs (N, cnum, k, masked, C) whose first draw leaves a named edge sample undecided, or more than half of
# CAP of the samples undecided, on the reference alone (tests/test_dpc_cpu.py: test_cap); every other input draws from its
# default seed.  Searched on the reference, default seed + 100003 n for the first n that passes.  Nearly all are k = 2: two mutual
# nearest neighbours have the same exponential term there, and fp32 orders them only when their noise draws lie some 0.03 apart
# -- at N = 64 a sample has about twenty such pairs and most draws leave most samples undecided.
RESEED = {
    (3, 1, 2, True, 64): 128722,
    (4, 1, 2, True, 512): 237092,
    (8, 3, 2, True, 512): 169027,
    (9, 3, 2, False, 1024): 177455,
    (9, 3, 2, True, 1024): 177458,
    (12, 3, 2, False, 512): 200700,
    (12, 3, 2, True, 256): 200447,
    (24, 4, 2, False, 512): 295859,
    (24, 4, 2, True, 512): 295862,
    (24, 24, 2, False, 64): 7998262,
    (24, 24, 2, False, 512): 498485,
    (24, 24, 2, True, 64): 898052,
    (24, 24, 5, True, 512): 298533,
    (32, 4, 2, False, 512): 959229,
    (32, 4, 2, False, 1024): 359723,
    (32, 4, 2, True, 512): 659223,
    (32, 4, 32, False, 1024): 460236,
    (33, 5, 2, False, 256): 1567041,
    (33, 5, 2, False, 512): 1467294,
    (33, 5, 2, True, 512): 767276,
    (62, 16, 5, False, 512): 1198422,
    (64, 11, 2, False, 512): 133617526,
    (64, 11, 2, True, 512): 913548,
    (64, 11, 3, False, 512): 613553,
    (64, 11, 5, False, 512): 813593,
    (64, 11, 5, True, 512): 613590,
    (64, 11, 64, False, 512): 120018172,
    (64, 11, 64, True, 512): 4514710,
    (64, 16, 2, False, 512): 203320272,
    (64, 16, 2, True, 512): 1014206,
    (64, 16, 3, True, 512): 614211,
    (64, 16, 5, False, 512): 914251,
    (64, 16, 64, False, 512): 424727968,
    (64, 16, 64, True, 512): 1715281,
}


def case_seed(N, cnum, k, masked, C):
    key = (N, cnum, k, masked, C)
    return RESEED.get(key, SEED + 7919 * N + 131 * cnum + 17 * k + 3 * int(masked) + C)


@functools.lru_cache(maxsize=None)
def random_tokens(N, cnum, k, masked, C=512):
    """-> (x [B,N,C] fp32: randn plus a shared component, layer-normed; mask [B,N] fp32 or None; noise [B,N] fp32)."""
    B = batch_of(N)
    g = torch.Generator().manual_seed(case_seed(N, cnum, k, masked, C))
    x = torch.randn(B, N, C, generator=g)
    x = torch.nn.functional.layer_norm(x + 0.5 * x[:, :1], (C,))
    mask = None
    if masked:
        mask = (torch.arange(N)[None] < mask_lengths(B, N, cnum, g)[:, None]).float()
    noise = torch.rand(B, N, generator=g)
    return x, mask, noise


def dist32_of(x):
    """fp64 distances rounded to fp32 (the CPU tests' matrix)."""
    xd = x.double()
    d = torch.cdist(xd, xd, compute_mode="donot_use_mm_for_euclid_dist") / math.sqrt(x.shape[-1])
    d = 0.5 * (d + d.transpose(1, 2))
    idx = torch.arange(x.shape[1])
    d[:, idx, idx] = 0
    return d.float()


# ---- (b) crafted distance matrices -------------------------------------------------------------------------------------------
# Eight active tokens on a line at dyadic positions (entries |p_i - p_j|: symmetric, zero diagonal, every square and every sum of
# k <= 5 squares exact), noise on the grid {0, 1/4, 1/2, 3/4}, the other tokens padding with raw entries RAW (overwritten by `far`
# in their columns, read raw in their rows).  Each named sample isolates one rule; the `mixed` samples draw positions with
# repeats from a pinned generator, so that several rules meet.
ACTIVE = 8
RAW = 4.0                                    # raw entries of padding rows / columns: the batch maximum, far = 5


def _line(pos):
    p = torch.tensor(pos, dtype=torch.float64)
    return (p[:, None] - p[None, :]).abs()


def _named(k):
    """name -> (active matrix [8,8], valid flags of the eight, noise of the eight in quarters, tight).  tight: the sample's padding
    entries are its own largest entry instead of RAW, so that its own maximum lies far below the batch's."""
    q = lambda *v: [x / 4 for x in v]
    allv = [1] * ACTIVE
    s = {}
    # token 0 at the same distance 1/4 from tokens 1..4 (three or more equal entries in its row), the rest spread out
    m = _line([0, 1, 1.125, 1.25, 1.375, 2.5, 3.0, 3.75])
    m[0, 1:5] = m[1:5, 0] = 0.25
    s["equal_row"] = (m, allv, q(0, 1, 2, 3, 0, 1, 2, 3), False)
    # tokens 2 and 3 are the same point: identical rows, equal exponential terms, ordered by their noise alone
    s["twin_rows"] = (_line([0, 0.25, 1, 1, 1.125, 2, 2.75, 3.5]), allv, q(1, 2, 0, 3, 2, 1, 0, 3), False)
    # ... and with the same noise: the same density bits, neither is denser than the other, both have the same score
    s["same_bits"] = (_line([0, 0.25, 1, 1, 1.125, 2, 2.75, 3.5]), allv, q(1, 2, 3, 3, 2, 1, 0, 0), False)
    # two isolated pairs, mirror images of each other with mirrored noise: token 1 and 2 tie for the densest and for the best
    # score, token 0 and 3 for the next
    s["equal_scores"] = (_line([0, 0.125, 3, 3.125, 3.5, 3.5, 3.5, 3.5]), [1, 1, 1, 1, 0, 0, 0, 0], q(1, 3, 3, 1, 0, 0, 0, 0), False)
    # token 2 half-way between the two densest groups: equidistant from two centres
    s["equidistant"] = (_line([0, 0.125, 1, 1.875, 2, 0.0625, 1.9375, 3.5]), [1, 1, 1, 1, 1, 1, 1, 0], q(3, 1, 0, 1, 2, 0, 0, 0), False)
    # token 1 is masked and sits right beside token 0: unmasked it would be 0's nearest neighbour and the densest pair
    s["masked_nearest"] = (_line([0, 0.03125, 0.5, 1.5, 1.75, 2.5, 3, 3.5]), [1, 0, 1, 1, 1, 1, 1, 1], q(0, 3, 1, 2, 3, 0, 1, 2), False)
    # a tight sample (largest entry 1/2, its padding rows included) in a batch whose maximum is 4: far = 5 against 1.5
    s["far"] = (_line([0, 0.125, 0.25, 0.375, 0.5, 0.0625, 0.3125, 0.4375]), [1, 1, 1, 1, 1, 0, 0, 0], q(0, 3, 1, 2, 0, 0, 0, 0), True)
    # every row the same point (one frame repeated, the padding too): all entries 0, the sample's maximum over real columns is 0
    # and only `far` gives the densest token a score above the others' 0
    s["all_zero"] = (_line([0] * ACTIVE), [1, 1, 1, 1, 0, 0, 0, 0], q(1, 0, 3, 2, 0, 0, 0, 0), True)
    # three valid tokens, tight: with k > 3 `far` itself is among the k nearest and its size weighs the exponential terms against
    # the noise -- token 0 and 1 are the densest pair, token 1 by the exponential term (by 48 / 65536 / k at k = 4), token 0 by
    # the noise, and far = 5 lets the noise win where far = 4 or 1.2 does not
    x, y, z = ((50, 40, 32) if k == 5 else (13, 11, 8))
    m = torch.zeros(ACTIVE, ACTIVE, dtype=torch.float64)
    m[0, 1] = z / 256
    m[0, 2] = x / 256
    m[1, 2] = y / 256
    m[:3, 3:] = x / 256
    m[3:, 3:] = x / 256
    m = torch.triu(m, 1)
    m = m + m.t()
    s["far_in_knn"] = (m, [1, 1, 1, 0, 0, 0, 0, 0], q(3, 0, 1, 0, 0, 0, 0, 0), True)
    return s


@functools.lru_cache(maxsize=None)
def crafted(N, k, cnum, n_mixed=7):
    """-> (dist [B,N,N] fp32, smax [B] fp32, mask [B,N] fp32, noise [B,N] fp32, names): every sample decided (asserted here; a
    mixed draw that is not decided on the reference is dropped before it is counted).  N > ACTIVE: the padding entries carry the
    batch maximum."""
    assert N > ACTIVE and k <= N
    g = torch.Generator().manual_seed(SEED + 1000 * N + 10 * k + cnum)
    items = [(name,) + v for name, v in _named(k).items()]
    tries = 0
    while len(items) < len(_named(k)) + n_mixed:
        tries += 1
        assert tries < 400
        pos = (torch.randint(0, 28, (ACTIVE,), generator=g).double() / 8).tolist()
        nv = int(torch.randint(2, ACTIVE + 1, (1,), generator=g))
        cand = (f"mixed{len(items)}", _line(pos), [1] * nv + [0] * (ACTIVE - nv),
                (torch.randint(0, 4, (ACTIVE,), generator=g).double() / 4).tolist(), False)
        d, _, mk, nz = _assemble(items + [cand], N)
        if bool(assign_ref(d, mk, nz, k, cnum).decided[-1]):
            items.append(cand)
    dist, smax, mask, noise = _assemble(items, N)
    ref = assign_ref(dist, mask, noise, k, cnum)
    names = tuple(it[0] for it in items)
    assert bool(ref.decided.all()), [n for n, ok in zip(names, ref.decided.tolist()) if not ok]
    return dist, smax, mask, noise, names


def _assemble(items, N):
    B = len(items)
    dist = torch.full((B, N, N), RAW, dtype=torch.float64)
    mask = torch.zeros(B, N)
    noise = torch.zeros(B, N)
    for b, (_, m, v, nzv, tight) in enumerate(items):
        if tight:
            dist[b] = float(m.max())
        dist[b, :ACTIVE, :ACTIVE] = m
        mask[b, :ACTIVE] = torch.tensor(v, dtype=torch.float32)
        noise[b, :ACTIVE] = torch.tensor(nzv, dtype=torch.float32)
    idx = torch.arange(N)
    dist[:, idx, idx] = 0
    dist = dist.float()
    return dist, dist.flatten(1).max(-1)[0], mask, noise


# ---- (c) repeated rows -------------------------------------------------------------------------------------------------------
def repeated_rows(B, N, C, seed):
    """Token sets with runs of bit-identical rows (repeated video frames) -> (x [B,N,C] fp32, noise [B,N] on the grid of quarters:
    a run of three duplicates at k = 3 has density 1 + noise * 1e-6, where fp32 tells quarters of the noise apart and little
    else).  Run lengths 1..4, drawn per sample."""
    g = torch.Generator().manual_seed(SEED + seed)
    x = torch.empty(B, N, C)
    for b in range(B):
        n = 0
        while n < N:
            run = min(int(torch.randint(1, 5, (1,), generator=g)), N - n)
            x[b, n:n + run] = torch.randn(C, generator=g)
            n += run
    x = x + 0.5 * x[:, :1]
    noise = torch.randint(0, 4, (B, N), generator=g).float() / 4
    return x, noise


# ---- the grouped launches of tests/test_dpc_gpu.py: (name, C, masked, ((N, cnum, k) of the text-shaped and the video-shaped problem)) ----
GROUPED = (
    ("m_form4", 512, True, ((24, 4, 3), (12, 3, 5))),
    ("m_form4_n32", 512, True, ((32, 4, 4), (12, 3, 3))),            # N = 32: the last shape of back form 4
    ("m_form16_n33", 512, True, ((33, 5, 5), (24, 4, 4))),           # N = 33: the first of back form 16
    ("m_form16", 512, True, ((64, 16, 4), (64, 11, 5))),             # token rows that do not fit the back half's LDS
    ("m_form1_c256", 256, True, ((24, 4, 3), (12, 3, 5))),
    ("m_form1_c24", 512, True, ((24, 24, 3), (12, 3, 4))),           # cnum = N > 16: the first form at C = 512
    ("u_few", 512, False, ((8, 3, 3), (4, 1, 2))),                   # N = 8: the last shape of the 256-thread fused kernel
    ("u_n9", 512, False, ((9, 3, 5), (3, 1, 3))),                    # N = 9: the first of the 512-thread one; k = N
    ("u_512", 512, False, ((24, 4, 3), (12, 3, 5))),
    ("u_512_n62", 512, False, ((62, 16, 5), (33, 5, 4))),           # N = 62: the most the fused second form can launch (below)
    ("u_form1_c256_few", 256, False, ((8, 3, 3), (4, 1, 4))),
    ("u_form1_c256", 256, False, ((24, 4, 5), (12, 3, 3))),
    ("u_form1_c24", 512, False, ((24, 24, 24), (12, 3, 3))),         # cnum = N and k = N
)
# kernel instantiations of the second-form back half that no shape reaches in a release build: with a mask the planner always
# finds room beside the kv GEMM at C = 512 (nr_linear_beside_back_fits: cnum <= back_form holds by the choice of back_form), and
# without one the stage is fused -- the launch of its own exists for NR_KV_APART (NR_TUNE builds)
UNREACHABLE = ("nr_group_back2_kernel<512, 4, 1>", "nr_group_back2_kernel<512, 16, 1>")


# channels of the stand-alone kernel's run of every shape (N * C * 4 above 64 KiB at N = 64, C = 512 and at 32 / 33 x 1024: the
# attribute path), and the (N, cnum, C) of the nr_ctm_front + nr_ctm_back runs (64 x 512: token rows that do not fit the LDS)
STANDALONE_C = {(3, 1): 64, (4, 1): 512, (8, 3): 64, (9, 3): 1024, (12, 3): 512, (24, 4): 512, (32, 4): 1024, (33, 5): 512,
                (64, 11): 512, (64, 16): 512, (24, 24): 64}
FRONT_BACK = ((24, 4, 512), (64, 16, 512), (12, 3, 256), (33, 5, 256))


def all_random_inputs():
    """(N, cnum, k, masked, C) of every random token set a test draws."""
    out = [(N, cnum, k, m, STANDALONE_C[(N, cnum)]) for N, cnum, k, m in random_cases()]
    out += [(N, cnum, k, m, C) for N, cnum, C in FRONT_BACK for n_, c_, k, m in random_cases() if (n_, c_) == (N, cnum)]
    out += [(N, cnum, k, masked, C) for _, C, masked, probs in GROUPED for N, cnum, k in probs]
    out += [(N, cnum, k, m, 512) for N, cnum, k, m in random_cases()]
    return sorted(set(out))


def crafted_cases():
    """(N, k, cnum) of every crafted batch a test feeds: the masked grouped problems, and nr_ctm_back at k = 3, 4, 5."""
    out = {(N, k, cnum) for _, _, masked, probs in GROUPED if masked for N, cnum, k in probs}
    return sorted(out | {(N, k, cnum) for N, cnum, _ in FRONT_BACK for k in (3, 4, 5)})


def ratio_of(N, cnum):
    """A sample_ratio with max(ceil(N * ratio), 1) == cnum."""
    r = (cnum - 0.5) / N
    assert max(math.ceil(N * r), 1) == cnum
    return r
