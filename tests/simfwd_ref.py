"""fp64 restatement of the fused similarity forward (modeling.py:499-512; nr_local_level_fwd) in stock torch:

    R[a, b, t, v] = <text token t of a, video token v of b>           (masked tokens are zero rows: their products are exactly 0)
    pmax[a, b, t] = max_v R,  arg_v = the FIRST v that attains it;    qmax[a, b, v] = max_t R,  arg_t = the first t
    S[a, b]       = 0.5 (sum_t w_t[a, t] pmax[a, b, t] + sum_v w_v[b, v] qmax[a, b, v])
    row form      = S.sum(1) (what the OUT_ROWSUM parts add up to),   column form = S.sum(0)

Two tiers, the same function `forward` on different operands:

  operand  the bf16 planes the kernel reads (`operands`: hi / lo as `prepare_tokens` splits them).  One pass: hi . hi.
           Split-bf16: hi . hi + hi . lo + lo . hi; lo . lo is NOT part of the plan.  What separates kernel and reference is the
           order and the precision (fp32) of the sums alone.
  exact    the fp32 inputs, normalised and masked in fp64 (`exact_terms`).

`forward` runs where `device` says (the GPU tests pass "cuda": R is [A, Bv, Nt, Nv]; stock torch, none of the project's kernels).
`twin` is the one measurement that sets the operand bars: the same formulas in plain fp32 on the CPU with every sum a sequential
loop (over k, over t, over v; vectorised over entries, no library reduction: torch's CPU matmul and sum change their blocking with
the host), on a fixed subsample of pairs that holds the first and the last, ragged, block and the masked samples.

Also here: the input makers, the table FORMS (case -> the plan nr_local_level_plan must report; pinned in test_simfwd_cpu.py,
asserted before every launch in test_simfwd_gpu.py) and the stored twin figures the bars are made of."""
import functools

import numpy as np
import torch

from neighborretr_amd import synth

# today's bars on S against fp64 of the exact inputs (tests/test_kernels_gpu.py): no bar of this file is looser
TODAY = {"bf16": 1e-3, "x3": 2e-6}
BAR_FACTOR = 8.0          # tree and MFMA summation order, the three-pass form's other order


def bf16_bits(t):
    """int16 tensor holding bf16 bit patterns (what the library hands around) -> the bf16 view of the same bytes."""
    return t.view(torch.bfloat16)


def split_bf16(x):
    """fp32 -> (hi, lo) bf16 bit patterns as int16, round to nearest even: hi = bf16(x), lo = bf16(x - hi)."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


def normalised(x, mask, normalize=True, dtype=torch.float64):
    """x [n, N, d] fp32, mask [n, N] -> normalize(x) * mask in fp64 (eps 1e-12 as F.normalize), [n, N, d]."""
    y = x.to(dtype)
    if normalize:
        y = y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return y * mask.to(dtype)[..., None]


def operands(x, mask, normalize=True):
    """CPU stand-in for ops.prepare_tokens: (hi, lo) int16 [n N, d] of the fp32 rounding of `normalised` (computed in fp64 and
    rounded once, so that the planes do not depend on the host's fp32 summation order).  Masked rows are exact zeros."""
    n, N, d = x.shape
    return split_bf16(normalised(x, mask, normalize).float().reshape(n * N, d))


def operand_terms(t_hi, t_lo, v_hi, v_lo, A, Nt, Bv, Nv, three):
    """The products the plan adds up, as [(T [A, Nt, d], V [Bv, Nv, d]), ...] in fp32 (bf16 values are exact in it)."""
    f = lambda p, n, N: bf16_bits(p).float().view(n, N, -1)
    Th, Vh = f(t_hi, A, Nt), f(v_hi, Bv, Nv)
    if not three:
        return [(Th, Vh)]
    Tl, Vl = f(t_lo, A, Nt), f(v_lo, Bv, Nv)
    return [(Th, Vh), (Th, Vl), (Tl, Vh)]


def exact_terms(t, tm, v, vm, normalize=True):
    return [(normalised(t, tm, normalize), normalised(v, vm, normalize))]


def first_max(R, dim):
    """(max, index of the FIRST maximum) along dim; torch.max leaves the index of a tie open."""
    m = R.amax(dim)
    n = R.shape[dim]
    shape = [1] * R.dim()
    shape[dim] = n
    ar = torch.arange(n, device=R.device).view(shape)
    idx = torch.where(R == m.unsqueeze(dim), ar, n).amin(dim)
    return m, idx


def forward(terms, w_t, w_v, device="cpu", budget=1 << 24, keep_R=False):
    """terms: [(T [A, Nt, d], V [Bv, Nv, d]), ...] whose products are summed; w_t [A, Nt], w_v [Bv, Nv].  Everything in fp64 on
    `device`.  -> dict S [A, Bv], rowsum [A], colsum [Bv], pmax / arg_v [A, Bv, Nt], qmax / arg_t [A, Bv, Nv] (and R if asked)."""
    A, Nt, _ = terms[0][0].shape
    Bv, Nv, _ = terms[0][1].shape
    terms = [(T.to(device=device, dtype=torch.float64), V.to(device=device, dtype=torch.float64)) for T, V in terms]
    w_t = w_t.to(device=device, dtype=torch.float64)
    w_v = w_v.to(device=device, dtype=torch.float64)
    step = max(1, budget // (Bv * Nt * Nv))
    out = {k: [] for k in ("S", "pmax", "arg_v", "qmax", "arg_t", "R")}
    for a0 in range(0, A, step):
        R = sum(torch.einsum("atd,bvd->abtv", T[a0:a0 + step], V) for T, V in terms)
        pm, av = first_max(R, 3)
        qm, at = first_max(R, 2)
        out["S"].append(0.5 * ((pm * w_t[a0:a0 + step, None, :]).sum(-1) + (qm * w_v[None]).sum(-1)))
        for k, x in (("pmax", pm), ("arg_v", av), ("qmax", qm), ("arg_t", at)):
            out[k].append(x)
        if keep_R:
            out["R"].append(R)
    res = {k: torch.cat(x) for k, x in out.items() if x}
    res["rowsum"], res["colsum"] = res["S"].sum(1), res["S"].sum(0)
    return res


def naive(terms, w_t, w_v):
    """The same function pair by pair in Python floats (doubles), first maximum by a strict `>` scan: tiny problems only."""
    import math
    A, Nt, d = terms[0][0].shape
    Bv, Nv, _ = terms[0][1].shape
    ts = [(T.double().tolist(), V.double().tolist()) for T, V in terms]
    wt, wv = w_t.double().tolist(), w_v.double().tolist()
    S = torch.zeros(A, Bv, dtype=torch.float64)
    pmax, arg_v = torch.zeros(A, Bv, Nt, dtype=torch.float64), torch.zeros(A, Bv, Nt, dtype=torch.int64)
    qmax, arg_t = torch.zeros(A, Bv, Nv, dtype=torch.float64), torch.zeros(A, Bv, Nv, dtype=torch.int64)
    for a in range(A):
        for b in range(Bv):
            R = [[math.fsum(T[a][t][k] * V[b][v][k] for T, V in ts for k in range(d)) for v in range(Nv)] for t in range(Nt)]
            s = 0.0
            for t in range(Nt):
                m, am = R[t][0], 0
                for v in range(1, Nv):
                    if R[t][v] > m:
                        m, am = R[t][v], v
                pmax[a, b, t], arg_v[a, b, t] = m, am
                s += wt[a][t] * m
            for v in range(Nv):
                m, am = R[0][v], 0
                for t in range(1, Nt):
                    if R[t][v] > m:
                        m, am = R[t][v], t
                qmax[a, b, v], arg_t[a, b, v] = m, am
                s += wv[b][v] * m
            S[a, b] = 0.5 * s
    return {"S": S, "pmax": pmax, "arg_v": arg_v, "qmax": qmax, "arg_t": arg_t}


def subsample(n):
    """The samples of an axis the twin runs on: the first three (1 or 2 of them is fully masked), the middle, the last two (the
    ragged block)."""
    return sorted({i for i in (0, 1, 2, n // 2, n - 2, n - 1) if 0 <= i < n})


def twin(terms, w_t, w_v):
    """`forward` in plain fp32 on the CPU, every sum a sequential loop; terms restricted by the caller to the subsample.
    -> dict R, pmax, qmax, S (fp32)."""
    T0, V0 = terms[0]
    A, Nt, d = T0.shape
    Bv, Nv, _ = V0.shape
    ts = [(T.float(), V.float()) for T, V in terms]
    R = torch.zeros(A, Bv, Nt, Nv, dtype=torch.float32)
    for k in range(d):
        for T, V in ts:
            R = R + T[:, None, :, None, k] * V[None, :, None, :, k]
    pm, qm = R.amax(3), R.amax(2)
    w_t, w_v = w_t.float(), w_v.float()
    t2v = torch.zeros(A, Bv, dtype=torch.float32)
    for t in range(Nt):
        t2v = t2v + pm[:, :, t] * w_t[:, None, t]
    v2t = torch.zeros(A, Bv, dtype=torch.float32)
    for v in range(Nv):
        v2t = v2t + qm[:, :, v] * w_v[None, :, v]
    return {"R": R, "pmax": pm, "qmax": qm, "S": 0.5 * (t2v + v2t)}


def measure(case):
    """Twin against fp64 on the subsample of one case's operand planes.  -> (e_R, e_S, bound_R, bound_S): the twin's largest
    error on a product sum (= on a pooled maximum) and on S, and the bounds that hold for ANY summation order:
    bound_R = 1.01 n 2^-24 max sum|a||b| over the n = K (x 3 terms) products of an entry; bound_S adds the (Nt + Nv + 1)-term
    weighted sums and the halving on maxima no larger than max sum|a||b| (the weights of a sample sum to 1)."""
    Nt, Nv, A, Bv, d, p = case
    x = make_inputs(case)
    sa, sb = subsample(A), subsample(Bv)
    terms = [(T[sa], V[sb]) for T, V in operand_terms(*x["planes"], A, Nt, Bv, Nv, p == "x3")]
    wt, wv = x["w_t"][sa], x["w_v"][sb]
    ref = forward(terms, wt, wv, keep_R=True)
    tw = twin(terms, wt, wv)
    e_R = float((tw["R"].double() - ref["R"]).abs().max())
    e_S = float((tw["S"].double() - ref["S"]).abs().max())
    mag = max(float(torch.einsum("atd,bvd->abtv", T.double().abs(), V.double().abs()).max()) for T, V in terms) * len(terms)
    n = d * len(terms)
    bound_R = 1.01 * n * 2.0 ** -24 * mag
    bound_S = bound_R + 1.01 * (Nt + Nv + 1) * 2.0 ** -24 * mag
    return e_R, e_S, bound_R, bound_S


def bars(p, d):
    """(bar on pmax / qmax / a product, bar on S) of the operand tier for precision p at width d: BAR_FACTOR x the twin's error
    (the largest over all cases of that precision), capped by the any-order bound at that width and by today's
    bar."""
    e_R, e_S = TWIN[p]
    bound_R, bound_S = BOUND[(p, d)]
    return min(BAR_FACTOR * e_R, bound_R, TODAY[p]), min(BAR_FACTOR * e_S, bound_S, TODAY[p])


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def masked_samples(A, Bv):
    """(fully masked text, fully masked video): inside the first block, never the last sample."""
    return (1 if A > 2 else None), (2 if Bv > 3 else (1 if Bv > 2 else None))


@functools.lru_cache(maxsize=4)
def make_inputs(case):
    """The random inputs of one case (the precision is not part of them): tokens base[i] + 4 eps as in test_kernels_gpu.py (text i
    and video i share a base: cosines of both signs, |cos| < 1), prefix masks of random length >= 1, ONE fully masked text and
    ONE fully masked video, token weights softmax(randn) over ALL tokens of a sample (masked ones included: their pooled maxima
    count).  -> dict t, v [n, N, d] fp32; tm, vm int64; w_t, w_v fp32; planes (t_hi, t_lo, v_hi, v_lo) int16."""
    Nt, Nv, A, Bv, d, _ = case
    seed, tag = 4100 + d, f"simfwd/{Nt}x{Nv}/{A}x{Bv}"
    base = synth.normal(seed, tag + "/base", (max(A, Bv), 1, d))
    t = _f32(base[:A] + 4.0 * synth.normal(seed, tag + "/t", (A, Nt, d)))
    v = _f32(base[:Bv] + 4.0 * synth.normal(seed, tag + "/v", (Bv, Nv, d)))
    tm = torch.from_numpy((np.arange(Nt)[None] < synth.randint(seed, tag + "/tm", 1, Nt, (A, 1))).astype(np.int64))
    vm = torch.from_numpy((np.arange(Nv)[None] < synth.randint(seed, tag + "/vm", 1, Nv, (Bv, 1))).astype(np.int64))
    ma, mb = masked_samples(A, Bv)
    if ma is not None:
        tm[ma] = 0
    if mb is not None:
        vm[mb] = 0
    w_t = torch.softmax(torch.from_numpy(synth.normal(seed, tag + "/wt", (A, Nt))), -1).float()
    w_v = torch.softmax(torch.from_numpy(synth.normal(seed, tag + "/wv", (Bv, Nv))), -1).float()
    planes = operands(t, tm) + operands(v, vm)
    return {"t": t, "v": v, "tm": tm, "vm": vm, "w_t": w_t, "w_v": w_v, "planes": planes}


@functools.lru_cache(maxsize=4)
def make_exact_inputs(case):
    """The tie tier's operands (`normalize = 0`): rows of at most 8 non-zeros, each a small integer in [-2, 2] times 2^-3; token
    weights k / 64 with k in [0, 4].  Every product is a multiple of 2^-6, |R| <= 1/2, every pooled term a multiple of 2^-12,
    |S| <= (Nt + Nv) / 64 <= 2 on a 2^-13 grid and a sum of up to 512 of them below 2^10: every sum is exact in fp32 in ANY order,
    and the values are bf16 numbers (lo is all zero).  Prefix masks; one fully masked text and video; and text 0 / the last
    text are POSITIVE on columns 0..7 while video 0 / the last video are NEGATIVE there, each with two or more masked tokens:
    every live product of those pairs is negative, so each of their maxima is the exact 0 of the masked tokens, a tie whose
    first index is the first masked token.  Same dict as make_inputs."""
    Nt, Nv, A, Bv, d, _ = case
    seed, tag = 5200 + d, f"simfwd-exact/{Nt}x{Nv}/{A}x{Bv}"

    def rows(n, N, name):
        val = synth.randint(seed, f"{tag}/{name}/val", -2, 2, (n, N, d)).astype(np.float64)
        rank = np.argsort(synth.uniform(seed, f"{tag}/{name}/pos", (n, N, d)), axis=-1)       # 8 random columns per row
        return np.where(rank < 8, val, 0.0) / 8.0

    def signed(n, N, name, sign):
        x = np.zeros((N, d))
        x[:, :8] = sign * synth.randint(seed, f"{tag}/{name}/{n}", 1, 2, (N, 8)) / 8.0
        return x

    t, v = rows(A, Nt, "t"), rows(Bv, Nv, "v")
    tm = (np.arange(Nt)[None] < synth.randint(seed, tag + "/tm", 1, Nt, (A, 1))).astype(np.int64)
    vm = (np.arange(Nv)[None] < synth.randint(seed, tag + "/vm", 1, Nv, (Bv, 1))).astype(np.int64)
    if Nt > 2 and Nv > 2:
        for a in {0, A - 1}:
            t[a] = signed(a, Nt, "pos", 1.0)
            tm[a] = np.arange(Nt) < max(1, Nt - 2 - a % 3)
        for b in {0, Bv - 1}:
            v[b] = signed(b, Nv, "neg", -1.0)
            vm[b] = np.arange(Nv) < max(1, Nv - 2 - b % 2)
    tm, vm = torch.from_numpy(tm), torch.from_numpy(vm)
    ma, mb = masked_samples(A, Bv)
    if ma is not None:
        tm[ma] = 0
    if mb is not None:
        vm[mb] = 0
    w_t = _f32(synth.randint(seed, tag + "/wt", 0, 4, (A, Nt)) / 64.0)
    w_v = _f32(synth.randint(seed, tag + "/wv", 0, 4, (Bv, Nv)) / 64.0)
    t, v = _f32(t), _f32(v)
    planes = operands(t, tm, normalize=False) + operands(v, vm, normalize=False)
    return {"t": t, "v": v, "tm": tm, "vm": vm, "w_t": w_t, "w_v": w_v, "planes": planes}


# ---- the launch forms of nr_local_level_fwd --------------------------------------------------------------------------------
# (Nt, Nv, A, Bv, d, precision, plan): plan = hip.local_level_plan(A, Nt, Bv, Nv, d, prec) =
#   (kernel, block rows, block columns, waves, ring depth, K loop, texts per block, videos per block, grid columns, grid rows,
#    lanes per pair of the LDS kernel), or None where the launch refuses.
# Derived with the plan call from nr_sim_reg_big / nr_pick_stages / nr_sim_reg_ring / nr_pick_extent / the LDS budget and pinned in
# tests/test_simfwd_cpu.py; if a picker changes, the case whose form it moved fails and this list has to be derived again.  Every
# shape is the smallest that reaches its form (block counts of exactly 256 = 16 x 16 or 529 = 23 x 23 >= 512) with the last block
# ragged on both axes wherever the form's threshold allows it.
_L0 = ("reg", 96, 96, 4, 2, "plain", 4, 8)
FORMS = [
    # 24 x 12 tokens.  96 x 96 blocks on the two-deep ring: one to eight K slices
    *[(24, 12, 5, 3, d, p, _L0 + (1, 2, 0)) for d in (64, 128, 192, 512) for p in ("bf16", "x3")],
    *[(24, 12, 37, 19, d, p, _L0 + (3, 10, 0)) for d in (64, 128, 192, 512) for p in ("bf16", "x3")],
    (24, 12, 92, 184, 128, "bf16", ("reg", 96, 96, 4, 1, "plain", 4, 8, 23, 23, 0)),          # one-deep ring: 529 workgroups
    (24, 12, 121, 241, 128, "bf16", ("reg", 192, 192, 8, 2, "pp", 8, 16, 16, 16, 0)),         # level 1
    (24, 12, 121, 241, 64, "bf16", ("reg", 192, 192, 8, 2, "plain", 8, 16, 16, 16, 0)),       # ... below K = 128: the plain loop
    (24, 12, 121, 241, 128, "x3", ("reg", 192, 192, 8, 1, "plain", 8, 16, 16, 16, 0)),        # ... split tile: one-deep ring
    (24, 12, 61, 241, 128, "x3", ("reg", 96, 192, 8, 2, "pp", 4, 16, 16, 16, 0)),             # level 3, 2 x 4 waves
    (24, 12, 61, 241, 64, "x3", ("reg", 96, 192, 4, 2, "plain", 4, 16, 16, 16, 0)),           # ... 2 x 2 waves below K = 128
    (24, 12, 121, 481, 128, "bf16", ("reg", 192, 384, 8, 2, "pp", 8, 32, 16, 16, 0)),         # level 2
    (24, 12, 121, 481, 64, "bf16", ("reg", 192, 384, 8, 2, "plain", 8, 32, 16, 16, 0)),
    (24, 12, 121, 481, 128, "x3", ("reg", 192, 384, 8, 2, "pp3", 8, 32, 16, 16, 0)),          # ... three accumulated passes
    (24, 12, 121, 481, 64, "x3", ("reg", 192, 384, 8, 2, "pp3", 8, 32, 16, 16, 0)),           # ... at ONE K slice
    # 64 x 64 tokens
    (64, 64, 3, 5, 128, "bf16", ("reg", 128, 128, 4, 2, "plain", 2, 2, 3, 2, 0)),
    (64, 64, 3, 5, 128, "x3", ("reg", 128, 128, 4, 2, "plain", 2, 2, 3, 2, 0)),
    (64, 64, 46, 46, 128, "x3", ("reg", 128, 128, 4, 1, "plain", 2, 2, 23, 23, 0)),
    (64, 64, 31, 64, 128, "bf16", ("reg", 128, 256, 8, 2, "pp", 2, 4, 16, 16, 0)),            # level 4
    (64, 64, 31, 64, 64, "bf16", ("reg", 128, 256, 8, 2, "plain", 2, 4, 16, 16, 0)),
    (64, 64, 64, 61, 128, "bf16", ("reg", 256, 256, 8, 2, "pp", 4, 4, 16, 16, 0)),            # level 5
    (64, 64, 64, 61, 128, "x3", ("reg", 256, 256, 8, 2, "pp3", 4, 4, 16, 16, 0)),
    (64, 64, 64, 61, 64, "bf16", ("reg", 256, 256, 8, 2, "pp", 4, 4, 16, 16, 0)),             # ... at one K slice
    (64, 64, 64, 61, 64, "x3", ("reg", 256, 256, 8, 2, "pp3", 4, 4, 16, 16, 0)),
    # 24 x 64 and 64 x 12 tokens
    (24, 64, 5, 3, 128, "bf16", ("reg", 96, 128, 4, 2, "plain", 4, 2, 2, 2, 0)),
    (24, 64, 5, 3, 128, "x3", ("reg", 96, 128, 4, 2, "plain", 4, 2, 2, 2, 0)),
    (24, 64, 92, 46, 128, "bf16", ("reg", 96, 128, 4, 1, "plain", 4, 2, 23, 23, 0)),
    (24, 64, 92, 46, 128, "x3", ("reg", 96, 128, 4, 1, "plain", 4, 2, 23, 23, 0)),
    (64, 12, 3, 21, 128, "bf16", ("reg", 128, 96, 4, 2, "plain", 2, 8, 3, 2, 0)),
    (64, 12, 3, 21, 128, "x3", ("reg", 128, 96, 4, 2, "plain", 2, 8, 3, 2, 0)),
    (64, 12, 46, 184, 128, "bf16", ("reg", 128, 96, 4, 1, "plain", 2, 8, 23, 23, 0)),
    (64, 12, 46, 184, 128, "x3", ("reg", 128, 96, 4, 1, "plain", 2, 8, 23, 23, 0)),
    # the LDS kernel: every (MI, NI) instance nr_pick_extent can return (96 / 128 rows x 96 / 128 columns), Nv % 4 == 0 and != 0,
    # 2 x 2 blocks with ragged second blocks; lanes per pair 1 (more than 256 pairs per block: several trips of phase C), 2, 4, 64
    *[(3, 6, 33, 17, 128, p, ("lds", 96, 96, 4, 2, "plain", 32, 16, 2, 2, 1)) for p in ("bf16", "x3")],
    *[(3, 7, 33, 19, 128, p, ("lds", 96, 128, 4, 2, "plain", 32, 18, 2, 2, 1)) for p in ("bf16", "x3")],
    *[(3, 8, 33, 17, 128, p, ("lds", 96, 128, 4, 2, "plain", 32, 16, 2, 2, 1)) for p in ("bf16", "x3")],
    *[(7, 6, 19, 17, 128, p, ("lds", 128, 96, 4, 2, "plain", 18, 16, 2, 2, 1)) for p in ("bf16", "x3")],
    *[(8, 12, 17, 9, 128, p, ("lds", 128, 96, 4, 2, "plain", 16, 8, 2, 2, 2)) for p in ("bf16", "x3")],
    *[(9, 20, 15, 7, 128, p, ("lds", 128, 128, 4, 2, "plain", 14, 6, 2, 2, 2)) for p in ("bf16", "x3")],
    *[(9, 20, 9, 11, 128, p, ("lds", 128, 128, 4, 2, "plain", 9, 6, 2, 1, 4)) for p in ("bf16", "x3")],
    *[(20, 7, 7, 19, 128, p, ("lds", 128, 128, 4, 2, "plain", 6, 18, 2, 2, 2)) for p in ("bf16", "x3")],
    (2, 2, 65, 65, 128, "bf16", ("lds", 128, 128, 4, 2, "plain", 64, 64, 2, 2, 1)),           # 4096 pairs: 16 trips of phase C
    (2, 2, 65, 65, 128, "x3", None),                                                          # 192 KiB of LDS: refused
    *[(128, 128, 3, 3, 128, p, ("lds", 128, 128, 4, 2, "plain", 1, 1, 3, 3, 64)) for p in ("bf16", "x3")],
    # one token per sample runs (128 samples per block edge) until 90 x 90 samples exceed the LDS budget; 129 tokens never do
    *[(1, 1, 5, 7, 128, p, ("lds", 128, 128, 4, 2, "plain", 5, 7, 1, 1, 4)) for p in ("bf16", "x3")],
    (1, 1, 90, 90, 128, "bf16", None),
    (129, 5, 2, 2, 128, "bf16", None),
    (5, 129, 2, 2, 128, "bf16", None),
]
CASES = [c[:6] for c in FORMS if c[6] is not None]
REFUSED = [c[:6] for c in FORMS if c[6] is None]


def _form_key(c):
    return (c[0], c[1]) + c[6][:6] + (c[5],)


def one_case_per_form():
    """The tie tier's cases: the first row of FORMS of every (token counts, kernel, block, waves, ring, loop, precision)."""
    seen, out = set(), []
    for c in FORMS:
        if c[6] is not None and _form_key(c) not in seen:
            seen.add(_form_key(c))
            out.append(c[:6])
    return out


# grouped launches (nr_local_level_group, d = 128): the smallest groupable product of each kind
GROUP_KIND = {0: (24, 12, 121, 481, 128, "bf16"), 1: (24, 12, 61, 241, 128, "x3")}

# ---- the twin's figures -------------------------------------------------------------------------------------------------
# TWIN[precision] = (e_R, e_S): the maxima of `measure` over ALL of CASES in that precision; BOUND[(precision, d)] = (bound_R,
# bound_S): its any-order bounds, the maxima over the cases of that width.  Stored with a tenth of headroom;
# tests/test_simfwd_cpu.py recomputes them and fails if a stored figure is under its measurement or over twice it.
TWIN = {"bf16": (9.784e-08, 3.490e-08), "x3": (2.721e-07, 1.193e-07)}
BOUND = {
    ("bf16", 64): (3.562e-06, 1.074e-05),
    ("bf16", 128): (6.895e-06, 1.984e-05),
    ("bf16", 192): (9.387e-06, 1.120e-05),
    ("bf16", 512): (2.402e-05, 2.576e-05),
    ("x3", 64): (3.126e-05, 5.226e-05),
    ("x3", 128): (6.206e-05, 9.907e-05),
    ("x3", 192): (8.449e-05, 8.991e-05),
    ("x3", 512): (2.162e-04, 2.214e-04),
}
