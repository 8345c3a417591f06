"""fp64 restatements of the step's FRONT END (csrc/nr_prepare.hip; nr_reduce_parts, nr_gemm_nt_f32, nr_centrality_weights[_pair]
of csrc/nr_small.hip; nr_colsum_group of csrc/nr_ctm_bwd.hip; nr_normalize_bwd of csrc/nr_backward.hip) and the makers of their
test inputs.  Plain torch on the CPU; nothing here calls the library.

Every function takes `dtype`: float64 is the reference, float32 the TWIN -- the same formulas in plain fp32 on the same inputs.
The twin's distance from the reference is what the arithmetic itself costs in fp32; the GPU tests' bars (tests/test_frontend_gpu.py)
are FACTOR times that, or a rigorous rounding bound where the operation is a pure sum, never anything measured on a kernel.
tests/test_frontend_cpu.py recomputes every E32_* / FRAC_* below on the inputs of every GPU case (the case lists below) and
holds the stored figures to them.

Inputs (make_tokens): rows of 3 randn; one exact-zero row, one row of norm 1e-14 (under F.normalize's 1e-12 clamp; every
element at least 1e-17, so its squares are normal fp32 numbers), samples of 4 tokens with prefix-ones masks of ragged length,
one sample fully masked."""
import math
from types import SimpleNamespace

import numpy as np
import torch

EPS = 1e-12                      # F.normalize's clamp (modeling.py:495)
FACTOR = 8.0                     # what the twin does not model: the kernels' summation orders, 1 / norm as a reciprocal, expf

# ---- tolerances ---------------------------------------------------------------------------------------------------------------
# E32_Y[d]: max over the preparation cases of width d of max|normalize_fp32(x) - normalize_fp64(x)| (absolute; |y| <= 1, the
# clamp row included).  The bars:  hi + lo: 2^-17 |ref| + FACTOR * E32_Y[d]  (two bf16 terms: |y - hi - lo| <= 2^-17 |y|);
# hi: 2^-8 |ref| + 1.01 * FACTOR * E32_Y[d]  (|y - hi| <= 2^-8 |y|).  With normalize = 0 the twin is exact (x * mask) and the
# bf16 terms stand alone.   measured 4.09e-8 / 3.23e-8 / 2.26e-8 / 2.24e-8
E32_Y = {256: 4.5e-8, 512: 3.6e-8, 768: 2.5e-8, 1024: 2.5e-8}
CAP_HILO, CAP_HI = 2e-5, 5e-3                        # tests/test_kernels_gpu.py::test_prepare_tokens
# relative error of the fp32 norm (rows above the clamp); measured 1.41e-7 / 1.62e-7 / 1.51e-7 / 1.81e-7
E32_NORM = {256: 1.6e-7, 512: 1.8e-7, 768: 1.7e-7, 1024: 2.0e-7}
CAP_NORM = 1e-4
# column sums of the unmasked normalised rows, absolute, by token-count class (1; under 64; 64 and more).  The bar of a column is
# the smaller of FACTOR * E32_COLSUM and the bound that holds for ANY order:
#   1.01 (n_tok + 1) 2^-24 sum|xn| + n_tok FACTOR E32_Y[d]     (summation + the element errors of the normalisation)
E32_COLSUM = {1: 2.3e-8, 16: 1.8e-7, 4096: 2.0e-6}          # measured 2.03e-8 / 1.61e-7 / 1.80e-6
CAP_COLSUM = 1e-4
# nr_gemm_nt_f32: the bar of an entry is min(1, FACTOR * FRAC_GEMM[K]) * gemm_bound; FRAC_GEMM[K] = max over the cases with that
# K and over entries of |twin - fp64| / gemm_bound.
FRAC_GEMM = {16: 0.16, 48: 0.066, 64: 0.045, 240: 0.0145, 256: 0.0135, 272: 0.011, 512: 0.0079, 1024: 0.0031}
CAP_GEMM = 2e-5                                      # * max|ref|: test_gemm_nt_f32's
# centrality weights w = mean_t exp(scale * cos_t), |scale * cos| < 1: absolute error of the twin; norms relative
E32_CW = 1.2e-7                                       # measured 1.08e-7; gnorm 1.53e-7, chain 5.77e-8, normalize_bwd 1.80e-7
CAP_CW = 1e-6                                        # test_centrality_weights'
E32_GNORM = 1.7e-7
# the chain prepare -> column sums -> weights from RAW features against the oracle (cosines of about 1 / sqrt(n_tok d))
E32_CW_CHAIN = 6.4e-8
# nr_normalize_bwd: per row, max|twin - fp64| / max|fp64 row|
E32_NBWD = 2.0e-7
CAP_NBWD = 1e-4


def bucket(n_tok):
    return 1 if n_tok == 1 else (16 if n_tok < 64 else 4096)


# ---- the GPU cases (tests/test_frontend_gpu.py runs exactly these; tests/test_frontend_cpu.py measures the twin on them) ------
PREP_D = [256, 512, 768, 1024]
# 1: three idle waves; 15 / 16 / 17: one part, one full part, a second part; 4096 / 4097: nr_prepare_parts reaches its cap of
# 256 workgroups = 1024 waves, so a wave's rows are 1024 apart and 4097 gives wave 0 of workgroup 0 a FIFTH row: the second trip
# of the batched-load loop for CH <= 2 (R = 4), the third for CH >= 3 (R = 2)
PREP_NTOK = [1, 15, 16, 17, 4096, 4097]
PREP_BIG = (32773, 256)          # without column sums: past the 2048-workgroup cap (2048 * 16 = 32768 tokens) by 5 rows
PREP_FLAG_SHAPE = (37, 512)      # the flag combinations
PAIR_SHAPES = [((5, 7), (3, 64)), ((16, 24), (16, 12)), ((4097, 1), (1, 1))]        # (samples, tokens) of the two tensors
PAIR_D = [256, 1024]
SPLIT_N = [1, 255, 256, 257, 2048 * 256 + 3]
GEMM_MN = [(1, 1), (1, 17), (15, 16), (17, 33), (37, 50)]
GEMM_K = [16, 48, 64, 240, 256, 272, 1024]
GEMM_PREFILTER = (7, 203, 512)
SUM_ROWS = [1, 3, 4, 5, 13, 16, 17, 29, 49, 64, 65, 113, 255, 256]
SUM_COLS = [1, 63, 64, 65, 512]
SUM_SCALE = 1.0 / 7              # rounded to fp32 before use (f32 below): the kernel multiplies by exactly that number
CW_SCALE = 0.3
CWP_B = [1, 3, 5, 9, 16]
CWP_G = [(1, 1), (3, 6), (1, 6)]
CWP_D = [256, 512, 1024, 68]
CWS_B = [1, 7, 8, 9, 17]
CWS_D = [256, 768, 1024]
CWS_PARTS = [1, 3, 4, 5, 17, 256]
CHAIN = [(5, 7, 24), (16, 24, 12)]                   # (B, Nt, Nv), d = 512
NBWD_NTOK = [1, 5, 96]
NBWD_D = [100, 256, 1024]
SEED = 5150


def f32(v):
    """The fp32 number nearest to v, as a Python float."""
    return float(np.float32(v))


# ---- the reference ------------------------------------------------------------------------------------------------------------
def normalize(x, dtype=torch.float64):
    """F.normalize: x / max(||x||, 1e-12) -> (xn, clamped norm [rows])."""
    x = x.to(dtype)
    nrm = x.norm(dim=-1).clamp_min(EPS)
    return x / nrm[:, None], nrm


def prepare(x, mask, normalize_flag=True, dtype=torch.float64):
    """x [n_tok, d], mask [n_tok] or None -> (y, norm, colsum): y = normalize(x) * mask (x * mask when normalize_flag is off),
    norm = max(||x||, 1e-12) either way, colsum [d] = the column sums of the UNMASKED rows of normalize(x) (of x): padding tokens
    count, modeling.py:413-424."""
    xn, nrm = normalize(x, dtype)
    if not normalize_flag:
        xn = x.to(dtype)
    y = xn if mask is None else xn * mask.to(dtype)[:, None]
    return y, nrm, xn.sum(0)


def split(y):
    """fp32 -> (hi, lo) int16 bit patterns: hi = bf16(y) round to nearest even, lo = bf16(y - hi).  torch's CPU conversion."""
    y = y.float()
    hi = y.to(torch.bfloat16)
    lo = (y - hi.float()).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


def bf(bits):
    """int16 bf16 bit patterns -> float64 values."""
    return bits.cpu().view(torch.bfloat16).double()


def gemm_nt(a, b, dtype=torch.float64):
    """A B^T.  float64: torch's matmul.  The fp32 TWIN adds the K products one after the other (c += a[:, k] b[:, k]^T, every
    product and every sum rounded once): the plain loop, and the same bits on every machine -- torch's fp32 CPU matmul changes
    its blocking with the thread count and the instruction set (its share of the rounding bound at K = 512 measured 0.0009 on
    one host and 0.0025 on another)."""
    if dtype == torch.float64:
        return a.double() @ b.double().t()
    a, b = a.to(dtype), b.to(dtype)
    c = torch.zeros(a.shape[0], b.shape[0], dtype=dtype)
    for k in range(a.shape[1]):
        c = c + a[:, k:k + 1] * b[:, k][None, :]
    return c


def gemm_bound(a, b):
    """Entry by entry: K products and K - 1 additions in any order, each rounded once."""
    K = a.shape[1]
    return 1.01 * K * 2.0 ** -24 * (a.double().abs() @ b.double().abs().t())


def reduce_parts(parts, scale, dtype=torch.float64):
    """scale * sum_p parts[p]  (until_module.py:181); `scale` is used as given in float64, rounded to fp32 in the twin."""
    return parts.to(dtype).sum(0) * scale


colsum = reduce_parts


def sum_bound(a, scale, n=None):
    """An n-term sum in any order followed by one multiplication: 1.01 (n + 1) 2^-24 |scale| sum|x|."""
    n = a.shape[0] if n is None else n
    return 1.01 * (n + 1) * 2.0 ** -24 * abs(scale) * a.double().abs().sum(0)


def centrality(g, mean, scale, dtype=torch.float64):
    """g [B, G, d], mean [d] -> (w [B], gnorm [B, G], wtok [B, G]): w_i = mean_t exp(scale <g_it, mean> / max(||g_it||, 1e-12))
    (modeling.py:403-430; G > 1: config.centrality_multi_token = "mean")."""
    g, mean = g.to(dtype), mean.to(dtype)
    gn = g.norm(dim=-1).clamp_min(EPS)
    wtok = torch.exp(scale * (g @ mean) / gn)
    return wtok.mean(-1), gn, wtok


def normalize_bwd(x, mask, d_xn, dmean, dtype=torch.float64):
    """d/dx of sum(d_xn * normalize(x) * mask) + sum(dmean * mean over ALL tokens of normalize(x)) by autograd in `dtype`; either
    cotangent may be None.  An exact-zero row gets g / 1e-12 (the norm's subgradient at 0 is 0, the clamp is constant)."""
    x = x.to(dtype).clone().requires_grad_()
    xn = x / x.norm(dim=-1, keepdim=True).clamp_min(EPS)
    total = 0.0
    if d_xn is not None:
        y = xn if mask is None else xn * mask.to(dtype)[:, None]
        total = total + (d_xn.to(dtype) * y).sum()
    if dmean is not None:
        total = total + (dmean.to(dtype) * xn.mean(0)).sum()
    total.backward()
    return x.grad


def row_rel_err(got, want):
    """max over rows of max|got - want| / max|want| of the row (rows whose reference is all zero: absolute)."""
    got, want = got.detach().double(), want.detach().double()
    den = want.abs().amax(-1)
    den = torch.where(den > 0, den, torch.ones_like(den))
    return float(((got - want).abs().amax(-1) / den).max())


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _normal(tag, shape):
    from neighborretr_amd import synth
    return synth.normal(SEED, "frontend/" + tag, shape)


def _uniform(tag, shape):
    from neighborretr_amd import synth
    return synth.uniform(SEED, "frontend/" + tag, shape)


def clamp_row(tag, d):
    """A row of norm 1e-14 whose elements are all at least 1e-14 / (3 sqrt(d)) in magnitude."""
    u = _uniform(tag + "/mag", (d,)) + 0.5
    s = np.where(_uniform(tag + "/sign", (d,)) < 0.5, -1.0, 1.0)
    r = u * s
    return r * (1e-14 / np.sqrt((r * r).sum()))


ZERO_ROW, CLAMP_ROW, MASKED_SAMPLE, SAMPLE = 2, 5, 2, 4       # rows 2 and 5, sample 2 = rows 8..11


def make_tokens(n_tok, d, variant=0, tag="prep"):
    """-> namespace(x [n_tok, d] fp32, mask [n_tok] fp32, zero, clamp: row indices or None).  n_tok >= 12: everything planted.
    n_tok = 1 has one row only; `variant` picks what it is: 0 an ordinary kept row, 1 the zero row, 2 the clamp row, 3 an
    ordinary MASKED row."""
    tag = f"{tag}/{n_tok}x{d}"
    x = 3.0 * _normal(tag + "/x", (n_tok, d))
    n_s = (n_tok + SAMPLE - 1) // SAMPLE
    length = np.minimum((_uniform(tag + "/len", (n_s,)) * SAMPLE).astype(np.int64) + 1, SAMPLE)        # 1 .. 4 kept tokens
    mask = (np.arange(SAMPLE)[None, :] < length[:, None]).astype(np.float64).reshape(-1)[:n_tok]
    q = SimpleNamespace(zero=None, clamp=None)
    if n_tok >= 12:
        q.zero, q.clamp = ZERO_ROW, CLAMP_ROW
        mask[MASKED_SAMPLE * SAMPLE:(MASKED_SAMPLE + 1) * SAMPLE] = 0.0
        mask[[ZERO_ROW, CLAMP_ROW]] = 1.0                            # both are KEPT rows: their outputs come from the clamp, not the mask
    else:
        assert n_tok == 1
        mask[0] = 0.0 if variant == 3 else 1.0
        q.zero = 0 if variant == 1 else None
        q.clamp = 0 if variant == 2 else None
    if q.zero is not None:
        x[q.zero] = 0.0
    if q.clamp is not None:
        x[q.clamp] = clamp_row(tag + "/clamp", d)
    q.x, q.mask = _t(x), _t(mask)
    return q


def make_pair(shape, d, which):
    """Tokens of one side of a pair case: shape = (samples, tokens per sample), prefix-ones masks of ragged length, the first
    sample of the first tensor fully masked, a zero row in the last sample."""
    n, N = shape
    tag = f"pair/{which}/{n}x{N}x{d}"
    x = 3.0 * _normal(tag + "/x", (n * N, d))
    length = np.minimum((_uniform(tag + "/len", (n,)) * N).astype(np.int64) + 1, N)
    mask = (np.arange(N)[None, :] < length[:, None]).astype(np.float64)
    if N == 1:
        mask = (_uniform(tag + "/len", (n, 1)) > 0.3).astype(np.float64)
    if which == 0 and n > 1:
        mask[0] = 0.0
    x[-1] = 0.0
    return SimpleNamespace(x=_t(x), mask=_t(mask.reshape(-1)))


def make_split(n):
    """fp32 values for nr_split_bf16: exact round-to-even ties of the bf16 conversion (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    ... and their negatives), +-0, magnitudes from 1e-30 to 1e30, randn elsewhere.  No subnormal, infinity or NaN."""
    special = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, 1e30, -1e30, 1e-30,
                        3 + 2.0 ** -7, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -24, 255.5, 256.0 + 1.0, 65280.0 + 128.0])
    v = _normal(f"split/{n}", (n,)) * np.exp(20.0 * (_uniform(f"split/{n}/e", (n,)) - 0.5))
    k = min(n, len(special))
    v[:k] = special[:k]
    if n > 600:
        v[-k:] = special[:k]                                                            # in the last, partial, block too
        v[300:300 + k] = special[:k] * 2.0 ** -20
    return _t(v)


def make_gemm(M, N, K):
    return _t(_normal(f"gemm/a/{M}x{K}", (M, K))), _t(_normal(f"gemm/b/{N}x{K}", (N, K)))


def make_sum(rows, cols, tag="sum"):
    """[rows, cols] fp32 of both signs: randn + 0.5."""
    return _t(_normal(f"{tag}/{rows}x{cols}", (rows, cols)) + 0.5)


def make_cw(B, G, d, tag):
    """(g [B, G, d], mean [d]): g_it = sqrt(d) c_it m + randn with c_it uniform in (-1, 0.1) and m = mean / ||mean||, so the
    cosines c / sqrt(1 + c^2) spread over about (-0.7, 0.1) (weights mostly below 1, where an fp32 ulp is 6e-8) instead of the +-1 / sqrt(d) of independent vectors; ||mean|| = 0.9 (a mean of unit rows has
    norm below 1) and |0.3 cos ||mean||| < 1.  Token 0 of sample 1 (of sample 0 when B = 1) is all zeros: weight exactly 1."""
    tag = f"cw/{tag}/{B}x{G}x{d}"
    m = _normal(tag + "/mean", (d,))
    m = m / np.sqrt((m * m).sum())
    c = 1.1 * _uniform(tag + "/c", (B, G, 1)) - 1.0
    g = math.sqrt(d) * c * m[None, None, :] + _normal(tag + "/g", (B, G, d))
    g[min(1, B - 1), 0] = 0.0
    return _t(g), _t(0.9 * m)


def make_cw_parts(n_parts, n_tok, d, tag):
    """[n_parts, d] fp32 partial column sums of n_tok tokens: every part is n_tok / n_parts times (m + noise of norm 0.3),
    ||m|| = 0.9, so their sum over n_tok is a mean of norm about 0.9 as the normalised tokens of a batch give."""
    tag = f"cws/{tag}/{n_parts}x{d}"
    m = _normal(tag + "/mean", (d,))
    m = 0.9 * m / np.sqrt((m * m).sum())
    parts = (m[None, :] + 0.3 / math.sqrt(d) * _normal(tag + "/p", (n_parts, d))) * (n_tok / n_parts)
    return _t(parts)


def make_cw_single(B, d, parts, n_tok, tag):
    """g [B, d] for the mean of `parts`, built like make_cw's; row 1 (row 0 when B = 1) is all zeros."""
    mean = parts.double().sum(0).numpy() / n_tok
    mh = mean / np.sqrt((mean * mean).sum())
    tag = f"cws/{tag}/g/{B}x{d}x{parts.shape[0]}"
    c = 1.1 * _uniform(tag + "/c", (B, 1)) - 1.0
    g = math.sqrt(d) * c * mh[None, :] + _normal(tag, (B, d))
    g[min(1, B - 1)] = 0.0
    return _t(g)


def make_chain(B, Nt, Nv, d=512):
    """Raw text / video token features, masks and one global token per sample: synth.make_samples (base + 6 randn) and randn."""
    from neighborretr_amd import synth
    t, v, tm, vm = synth.make_samples(SEED, f"frontend/chain/{B}", B, Nt, Nv, d)
    gt, gv = _t(_normal(f"chain/gt/{B}", (B, 1, d))), _t(_normal(f"chain/gv/{B}", (B, 1, d)))
    return SimpleNamespace(text=torch.from_numpy(t), video=torch.from_numpy(v), tm=torch.from_numpy(tm), vm=torch.from_numpy(vm),
                           gt=gt, gv=gv)


def chain(q, scale, dtype=torch.float64):
    """The step's chain in `dtype`: normalise every token, mean over ALL tokens, centrality weights -> (w_text, w_video)."""
    out = []
    for x, g in ((q.text, q.gt), (q.video, q.gv)):
        xn, _ = normalize(x.reshape(-1, x.shape[-1]), dtype)
        out.append(centrality(g, xn.mean(0), scale, dtype)[0])
    return out


def make_nbwd(n_tok, d):
    """x (row 0 masked; row 1 exactly zero when n_tok > 1), mask, d_xn, dmean for nr_normalize_bwd.  No row has a norm in
    (0, 1e-12): there the kernel projects and the clamp's derivative does not -- out of scope, asserted neither way."""
    tag = f"nbwd/{n_tok}x{d}"
    x = 3.0 * _normal(tag + "/x", (n_tok, d))
    mask = (_uniform(tag + "/m", (n_tok,)) > 0.3).astype(np.float64)
    mask[0] = 0.0
    if n_tok > 1:
        x[1] = 0.0
        mask[1] = 1.0
    return SimpleNamespace(x=_t(x), mask=_t(mask), d_xn=_t(_normal(tag + "/d_xn", (n_tok, d))), dmean=_t(_normal(tag + "/dmean", (d,))))
