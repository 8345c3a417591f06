"""fp64 restatement of the split-bf16 linear engine (csrc/nr_linear.hip on csrc/nr_gemm_tile.h: nr_linear_group, nr_linear_x3),
the makers of its test inputs, the case lists of tests/test_linear_gpu.py and the bars.  Plain torch; nothing here calls the
library.  The functions work on whatever device their tensors are on (the GPU tests compute the fp64 side on the device).

REFERENCE.  The fp64 product of the split operands AS THE KERNEL SEES THEM: (hi + lo) of X times (hi + lo) of W, plus bias, plus
residual -- the error of the split itself is not the engine's and stays out.  Conv form: sum_s X[r + s - 1] . W[:, s K/3 :
(s + 1) K/3] with the rows outside r's sample of conv_n tokens read as zeros (expand()).  One-pass form: the hi halves only.

TWIN.  The same three products (Al Bh, Ah Bl, Ah Bh; one for the one-pass form) in plain fp32, slice of 64 by slice of 64: inside
a slice every product is a sequential sum (each multiplication and each addition rounded once, the plain loop: the same bits on
every machine), the slice's products are then added to the accumulator one after the other.

BARS, entry by entry.  A = |X| |W|^T, A_ll = |X_lo| |W_lo|^T (the lo * lo term the engine drops by design), n_ops = 3 K for the
split form and K for one pass, ULP = 2^-23 |prod + bias| (bias given) + 2^-23 |ref| (residual given): the two fp32 additions of
the epilogue, each rounded once.
  rigorous   A_ll + 1.01 n_ops 2^-23 A + ULP      asserted on EVERY case.  Holds for any summation order and any rounding mode at
             one rounding per operation (2^-23, not 2^-24: how the matrix cores round inside an accumulation is not documented).
  working    A_ll + min(1, FACTOR FRAC[K]) 1.01 n_ops 2^-24 A + ULP      asserted on the randn cases.  FRAC[K] = the largest
             entry of |twin - ref3| / (1.01 n_ops 2^-24 A) over the randn problems with that K, ref3 = the fp64 sum of the products
             the engine keeps (the reference without lo * lo: that term has its own place in the bar) -- measured on the CPU by
             tests/test_linear_cpu.py, which holds the stored figures to what it measures; never taken from a kernel.
Coherent inputs (hi random positive bf16, lo = hi 2^-10 exactly, for X and for W): every cross term adds with one sign, so a
dropped Ah Bl or Al Bh pass is 2^-10 of the value, far outside the rigorous bar (on random signs it shrinks like 1 / sqrt(K) and
at K = 1536 sits at about the rounding bound)."""
import zlib
from types import SimpleNamespace
from typing import NamedTuple

import torch

import frontend_ref

FACTOR = frontend_ref.FACTOR                 # 8: what the twin does not model -- the matrix cores' summation order inside a product
NAN16 = 0x7FC0                               # the bf16 quiet NaN as an int16 bit pattern
SENT32 = 0x5A5A5A5A                          # sentinel of the output buffers as an int32 bit pattern (1.5e16 as fp32)
SEED = 6150
TWIN_ROWS = 192                              # problems of more than 2^17 outputs: the twin runs on this many rows spread over M

# share of the any-order 2^-24 bound the twin uses, by K (see above); it falls like 1 / K: the bound grows like K^2 (K terms times
# a sum of K magnitudes), a sequential sum's error on random signs like K
#        measured 0.0159 / 0.00502 / 0.00356 / 0.00134 / 0.00106 / 0.00104 / 0.000421 / 0.000226
FRAC3 = {64: 0.018, 128: 0.0057, 192: 0.004, 256: 0.0015, 320: 0.0012, 384: 0.0012, 512: 0.00048, 1536: 0.00026}
#        one pass: measured 0.033 / 0.0109 / 0.00604 / 0.000235
FRAC1 = {64: 0.037, 128: 0.0125, 192: 0.0068, 1536: 0.00027}


class P(NamedTuple):
    """One problem Y[M, N] = X[M, K] W[N, K]^T (+ bias) (+ residual).  ld > 0: X and W are K-slices at column `off` of matrices of
    row pitch ld.  conv_n > 0: X is the token matrix [M, K / 3] in samples of conv_n rows."""
    M: int
    N: int
    K: int
    bias: int = 0
    res: int = 0
    ld: int = 0
    off: int = 0
    conv_n: int = 0


class Case(NamedTuple):
    """One launch.  family: "group" (nr_linear_group) or "x3" (nr_linear_x3, one problem); kind: "randn" or "coh"; variant: the
    (MI, NI, STAGES, WC, conv, one_pass) the dispatcher is expected to pick (tests/test_linear_cpu.py asks the plan function)."""
    name: str
    family: str
    kind: str
    one_pass: bool
    probs: tuple
    variant: tuple


# ---- every kernel instantiation a release build holds (csrc/nr_linear.hip), and the ones no shape reaches -------------------------
INSTANTIATIONS = {
    "group": {(1, 2, 4, 2, 0, 0), (1, 2, 2, 2, 0, 0), (2, 2, 1, 2, 0, 0), (2, 2, 1, 4, 0, 0), (4, 4, 1, 2, 0, 0),
              (1, 2, 4, 2, 1, 0), (1, 2, 2, 2, 1, 0), (2, 2, 1, 2, 1, 0),
              (2, 2, 1, 4, 0, 1), (2, 2, 2, 4, 0, 1), (2, 2, 1, 2, 0, 1), (2, 2, 2, 2, 0, 1)},
    "x3": {(4, 4, 1, 2, 0, 0), (4, 4, 2, 2, 0, 0), (2, 4, 1, 2, 0, 0), (2, 4, 2, 2, 0, 0)},
}
# one pass on 4 waves has t32x64 < 1024 and a one-deep ring needs t32x64 / 2 >= 512; nr_linear_x3's 64 x 128 block has at most
# 2 * 191 workgroups and a one-deep ring needs 512
UNREACHABLE = {("group", (2, 2, 1, 2, 0, 1)), ("x3", (2, 4, 1, 2, 0, 0))}


def block(variant):
    """(BM, BN) of a variant."""
    mi, ni, _, wc = variant[:4]
    return 32 * mi, 16 * wc * ni


# ---- the cases ------------------------------------------------------------------------------------------------------------------
G124, G122, G221, G228, G441 = (1, 2, 4, 2, 0, 0), (1, 2, 2, 2, 0, 0), (2, 2, 1, 2, 0, 0), (2, 2, 1, 4, 0, 0), (4, 4, 1, 2, 0, 0)
C124, C122, C221 = (1, 2, 4, 2, 1, 0), (1, 2, 2, 2, 1, 0), (2, 2, 1, 2, 1, 0)
O222, O228, O218 = (2, 2, 2, 2, 0, 1), (2, 2, 2, 4, 0, 1), (2, 2, 1, 4, 0, 1)
X242, X442, X441 = (2, 4, 2, 2, 0, 0), (4, 4, 2, 2, 0, 0), (4, 4, 1, 2, 0, 0)
FLAGS = ((0, 0), (1, 0), (0, 1), (1, 1))
CONV_N = (1, 2, 3, 31, 32, 33, 64, 65)
# rows of the conv problems: whole samples (the callers' relation: M = n_samples * conv_n -- a partial last sample would make
# its last row read the row behind the matrix), about two 32-row blocks each; 32: samples ending exactly on a block edge;
# 33 / 65: samples that span two and three blocks; 31: a sample boundary one row in front of a block edge
CONV_SAMPLES = {1: 33, 2: 17, 3: 11, 31: 2, 32: 2, 33: 2, 64: 1, 65: 1}


def edges(variant, K, one_pass=False):
    """Problems at the block edges of a variant: M in {1, BM - 1, BM, BM + 1}, N in {1, 15, 16, 17, BN - 1, BN + 1} (16-column
    sub-tile edges inside a wave's strip among them), and one of a few blocks each way; mixed flags."""
    BM, BN = block(variant)
    shapes = [(1, 1), (BM - 1, 15), (BM, 16), (BM + 1, 17), (BM + 1, BN - 1), (BM - 1, BN + 1), (2 * BM + 1, 2 * BN + 1)]
    return [P(m, n, K, *FLAGS[i % 4]) for i, (m, n) in enumerate(shapes)]


def _flags(M, N, K, **kw):
    return tuple(P(M, N, K, b, r, **kw) for b, r in FLAGS)


def _conv_probs(C, N, flags=True):
    return [P(CONV_SAMPLES[n] * n, N, 3 * C, *(FLAGS[i % 4] if flags else (0, 0)), conv_n=n) for i, n in enumerate(CONV_N)]


def _build_cases():
    cs = []
    add = lambda name, family, kind, one, probs, variant: cs.append(Case(name, family, kind, one, tuple(probs), variant))
    g = lambda name, kind, probs, variant, one=False: add(name, "group", kind, one, probs, variant)

    # -- non-conv, split-bf16.  <1,2,4>: at most 256 tiles of 32 x 64; the 4-deep ring with fewer slices than stages, as many, more
    g("g124/edges", "randn", edges(G124, 64) + [P(32, 64, 64, 1, 1)], G124)
    for K in (64, 128, 192, 256, 320):
        for kind in ("randn", "coh"):
            g(f"g124/flags/K{K}/{kind}", kind, _flags(33, 65, K), G124)
    g("g124/K1536", "randn", [P(33, 65, 1536, 1, 1)], G124)
    g("g124/K512", "randn", [P(33, 65, 512, 0, 1)], G124)
    g("g124/K512/coh", "coh", [P(33, 65, 512, 1, 0)], G124)
    # <1,2,2>: 257 .. 640 tiles: a filler of 17 x 16 tiles beside the edge problems; the 2-deep ring at 1, 2, 3 slices
    for K in (64, 128, 192):
        g(f"g122/edges/K{K}", "randn", [P(513, 961, K, 1, 0)] + edges(G122, K), G122)
    for kind in ("randn", "coh"):
        g(f"g122/flags/{kind}", kind, _flags(257, 961, 128), G122)
    # <2,2,1> on 4 waves: 641 .. 1536 tiles
    for K in (64, 128):
        g(f"g221/edges/K{K}", "randn", [P(1281, 961, K, 0, 1)] + edges(G221, K), G221)
    for kind in ("randn", "coh"):
        g(f"g221/flags/{kind}", kind, _flags(449, 961, 128), G221)
    # <2,2,1> on 8 waves (64 x 128): more than 1536 tiles of 32 x 64, fewer than 1024 of 128 x 128; a K-slice problem among them
    for K in (64, 128):
        g(f"g228/edges/K{K}", "randn", [P(3073, 1025, K, 1, 0)] + edges(G228, K)[:6] + [P(65, 129, K, 1, 1, ld=K + 64, off=64)], G228)
    for kind in ("randn", "coh"):
        g(f"g228/flags/{kind}", kind, _flags(769, 1025, 128), G228)
    # <4,4,1> (128 x 128): 1024 tiles of 128 x 128 and more
    g("g441/edges", "randn", [P(4090, 4090, 64, 1, 0)] + edges(G441, 64), G441)
    for kind in ("randn", "coh"):
        g(f"g441/flags/{kind}", kind, _flags(2041, 2049, 64), G441)

    # -- the k=3 token convolution read in place
    for C in (64, 128, 512):
        g(f"c124/C{C}", "randn", _conv_probs(C, C), C124)
    g("c124/odd_N", "randn", _conv_probs(64, 65), C124)
    for kind in ("randn", "coh"):
        g(f"c124/flags/{kind}", kind, _flags(72, 64, 192, conv_n=24), C124)
    for C in (64, 128):
        g(f"c122/C{C}", "randn", [P(528, 961, 3 * C, 1, 0, conv_n=24)] + _conv_probs(C, 65)[:7], C122)
        g(f"c221/C{C}", "randn", [P(1284, 961, 3 * C, 0, 0, conv_n=12)] + _conv_probs(C, 65)[:7], C221)
    g("c122/flags/coh", "coh", _flags(264, 961, 192, conv_n=24), C122)
    g("c221/flags/coh", "coh", _flags(444, 961, 192, conv_n=12), C221)
    g("c221/big", "randn", [P(3072, 1025, 192, 1, 0, conv_n=24), P(65, 64, 192, 0, 0, conv_n=65)], C221)      # past 1536 tiles: the same blocks

    # -- one pass (hi halves only)
    o = lambda name, kind, probs, variant: g(name, kind, probs, variant, True)
    for K in (64, 128, 192):
        o(f"o222/edges/K{K}", "randn", edges(O222, K) + [P(100, 100, K, 1, 1)], O222)
    for kind in ("randn", "coh"):
        o(f"o222/flags/{kind}", kind, _flags(65, 65, 128), O222)
    o("o222/K1536", "randn", [P(65, 129, 1536, 1, 1)], O222)
    for K in (64, 128, 192):
        o(f"o228/edges/K{K}", "randn", [P(2049, 1025, K, 1, 0)] + edges(O228, K), O228)
    o("o228/flags/coh", "coh", _flags(513, 1025, 128), O228)
    for K in (64, 128):
        o(f"o218/edges/K{K}", "randn", [P(4097, 1025, K, 0, 1)] + edges(O218, K)[:6] + [P(65, 129, K, 1, 1, ld=4 * K, off=2 * K)], O218)
    o("o218/flags/coh", "coh", _flags(1025, 1025, 128), O218)

    # -- row pitch: K-slices of wider matrices at column offsets that are multiples of 64, ld in {K + 8, K + 64, 4 K}
    K = 128
    ldp = [P(65, 129, K, 1, 0, ld=K + 8, off=0), P(65, 129, K, 0, 1, ld=K + 64, off=64), P(33, 65, K, 1, 1, ld=4 * K, off=K),
           P(31, 17, K, 0, 0, ld=4 * K, off=3 * K)]
    g("ld/split", "randn", ldp, G124)
    o("ld/one", "randn", ldp, O222)
    g("ld/split/coh", "coh", ldp, G124)

    # -- groups: eight different (M, N, K) with mixed flags; a one-tile problem between large ones; 1, 7, 8, 9 tiles in all (the
    # padding workgroups of the XCD order); eleven problems for the chunking of the Python caller
    g("grp/mixed8", "randn", MIXED8, G124)
    g("grp/one_tile_between", "randn", [P(300, 500, 64, 1, 0), P(5, 7, 128, 0, 1), P(290, 520, 64, 1, 1)], G124)
    g("grp/tiles1", "randn", [P(20, 40, 64, 1, 1)], G124)
    g("grp/tiles7", "randn", [P(33, 129, 64, 1, 0), P(5, 5, 64, 0, 1)], G124)
    g("grp/tiles8", "randn", [P(64, 256, 64, 0, 1)], G124)
    g("grp/tiles9", "randn", [P(65, 129, 64, 1, 1)], G124)

    # -- nr_linear_x3: 64 x 128 blocks on a 2-deep ring; 128 x 128 from 192 tiles of 128 x 128, one-deep from 512 workgroups
    x = lambda name, kind, p, variant: add(name, "x3", kind, False, [p], variant)
    for i, p in enumerate(edges(X242, 64) + [P(200, 130, 64, 1, 1)]):
        x(f"x242/edge{i}", "randn", p, X242)
    for K in (128, 192):
        x(f"x242/K{K}", "randn", P(65, 129, K, 1, 0), X242)
    for i, p in enumerate(_flags(65, 129, 128)):
        x(f"x242/flags{i}/randn", "randn", p, X242)
        x(f"x242/flags{i}/coh", "coh", p, X242)
    x("x242/K1536", "randn", P(65, 129, 1536, 1, 1), X242)
    for v, tag, M in ((X442, "x442", 1409), (X441, "x441", 3969)):
        for K in (64, 192):
            x(f"{tag}/K{K}", "randn", P(M, 2049, K, 1, 0), v)
        for i, p in enumerate(_flags(M, 2049, 128)):
            x(f"{tag}/flags{i}/randn", "randn", p, v)
            x(f"{tag}/flags{i}/coh", "coh", p, v)
    return cs


MIXED8 = [P(33, 65, 64, 1, 0), P(1, 130, 128, 0, 1), P(70, 17, 192, 1, 1), P(64, 64, 256, 0, 0), P(95, 200, 320, 1, 0), P(200, 30, 64, 0, 1),
          P(17, 17, 512, 1, 1), P(129, 65, 128, 0, 0)]
CHUNKED11 = MIXED8 + [P(31, 63, 64, 1, 1), P(64, 128, 128, 0, 0), P(2, 300, 192, 1, 0)]
CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def plan_args(case, probs=None):
    """The problems of a case in the form hip.linear_plan takes."""
    return [(p.M, p.N, p.K, p.ld, p.conv_n, case.one_pass) for p in (case.probs if probs is None else probs)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def split(y):
    """fp32 -> (hi, lo) int16 bit patterns: hi = bf16(y) round to nearest even, lo = bf16(y - hi)."""
    return frontend_ref.split(y)


def _draw(fn, tag, shape):
    from neighborretr_amd import synth
    return torch.from_numpy(getattr(synth, fn)(SEED, "linear/" + tag, shape)).float()


def make_inputs(case, i):
    """Problem i of a case on the CPU -> namespace(xh, xl, wh, wl: int16 bf16 bit patterns, X [M, K] ([M, K / 3] for a conv), W
    [N, K]; xl = wl = None for one pass; bias [N] / res [M, N] fp32 or None).  Made from the case's name: the operands by the
    counter-based generator of neighborretr_amd.synth (the same bits on every machine and library version: the stored FRAC figures
    are measured on them), bias and residual by torch's CPU generator.
    randn: X = randn, W = 0.05 randn, split.  coh: hi = bf16(0.5 + uniform), lo = hi 2^-10 exactly, for X and for W."""
    p = case.probs[i]
    tag = f"{case.name}/{i}"
    kx = p.K // 3 if p.conv_n else p.K
    if case.kind == "randn":
        xh, xl = split(_draw("normal", tag + "/x", (p.M, kx)))
        wh, wl = split(_draw("normal", tag + "/w", (p.N, p.K)) * 0.05)
    else:
        def coh(which, r, c):
            hi = (0.5 + _draw("uniform", tag + which, (r, c))).to(torch.bfloat16)
            lo = (hi.float() * 2.0 ** -10).to(torch.bfloat16)
            assert torch.equal(lo.double(), hi.double() * 2.0 ** -10)
            return hi.view(torch.int16), lo.view(torch.int16)
        xh, xl = coh("/x", p.M, kx)
        wh, wl = coh("/w", p.N, p.K)
    if case.one_pass:
        xl = wl = None
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    bias = torch.randn(p.N, generator=g) if p.bias else None
    res = torch.randn(p.M, p.N, generator=g) if p.res else None
    return SimpleNamespace(xh=xh, xl=xl, wh=wh, wl=wl, bias=bias, res=res)


# ---- reference, twin, bars ------------------------------------------------------------------------------------------------------
def _val(bits, dtype):
    return bits.view(torch.bfloat16).to(dtype)


def expand(x, conv_n, taps=(-1, 0, 1), cross=False):
    """Token rows x [M, C] in samples of conv_n rows -> [M, 3 C]: segment s holds x[r + taps[s]], zeros where that row lies
    outside the sample of r (outside the matrix only, with cross = True: a planted defect, like taps other than -1, 0, 1)."""
    M = x.shape[0]
    r = torch.arange(M, device=x.device)
    t = r % conv_n
    segs = []
    for d in taps:
        src = r + d
        on = (src >= 0) & (src < M)
        if not cross:
            on = on & (t + d >= 0) & (t + d < conv_n)
        segs.append(torch.where(on[:, None], x[src.clamp(0, M - 1)], torch.zeros_like(x)))
    return torch.cat(segs, 1)


def operands(p, q, dtype, taps=(-1, 0, 1), cross=False):
    """(Xh, Xl, Wh, Wl) as [M, K] / [N, K] matrices of `dtype` (the conv's token rows expanded); Xl = Wl = None for one pass."""
    out = []
    for hi, lo in ((q.xh, q.xl), (q.wh, q.wl)):
        out += [_val(hi, dtype), None if lo is None else _val(lo, dtype)]
    if p.conv_n:
        out[0] = expand(out[0], p.conv_n, taps, cross)
        out[1] = None if out[1] is None else expand(out[1], p.conv_n, taps, cross)
    return out


def reference(p, q, frac=None):
    """-> namespace(ref; ref3 = ref without the lo * lo product, prod3 = ref3 without bias and residual; a_ll, unit = 1.01 n_ops
    2^-24 A; rigorous, working) in fp64 on the device of q's tensors.  frac: FRAC[K] of the working bar (None:
    the stored figure of this K; the working bar is None where no figure is stored)."""
    Xh, Xl, Wh, Wl = operands(p, q, torch.float64)
    one = Xl is None
    X, W = (Xh, Wh) if one else (Xh + Xl, Wh + Wl)
    prod = X @ W.t()
    A = X.abs() @ W.abs().t()
    if one:
        A_ll, ll = torch.zeros_like(A), torch.zeros_like(A)
    else:
        A_ll, ll = Xl.abs() @ Wl.abs().t(), Xl @ Wl.t()
    ref, ulp = prod, torch.zeros_like(A)
    if q.bias is not None:
        ref = ref + q.bias.double()[None, :]
        ulp = ulp + 2.0 ** -23 * ref.abs()
    if q.res is not None:
        ref = ref + q.res.double()
        ulp = ulp + 2.0 ** -23 * ref.abs()
    n_ops = p.K if one else 3 * p.K
    unit = 1.01 * n_ops * 2.0 ** -24 * A
    if frac is None:
        frac = (FRAC1 if one else FRAC3).get(p.K)
    working = None if frac is None else A_ll + min(1.0, FACTOR * frac) * unit + ulp
    return SimpleNamespace(ref=ref, ref3=ref - ll, prod3=prod - ll, a_ll=A_ll, unit=unit, rigorous=A_ll + 2.0 * unit + ulp, working=working)


def twin_rows(p):
    """The rows the twin runs on: all of them, or TWIN_ROWS spread over M (first and last included) for a large problem."""
    if p.M * p.N <= 2 ** 17:
        return torch.arange(p.M)
    return torch.unique(torch.linspace(0, p.M - 1, TWIN_ROWS).round().long())


def twin(p, q, rows=None, drop=None, skip_last=False, bias_shift=0, taps=(-1, 0, 1), cross=False, epilogue=True):
    """The engine's arithmetic in plain fp32 on the CPU (see the top of the file) for the given rows -> [len(rows), N] fp32.
    Planted defects: drop = "lh" / "hl" leaves that cross product out; skip_last leaves the last K slice out; bias_shift takes
    the bias of column c + bias_shift (cyclically); taps / cross: see expand.  epilogue = False: the product alone."""
    Xh, Xl, Wh, Wl = operands(p, q, torch.float32, taps, cross)
    rows = torch.arange(p.M) if rows is None else rows
    Xh = Xh[rows].contiguous()
    pairs = [(Xh, Wh)]
    if Xl is not None:
        Xl = Xl[rows].contiguous()
        pairs = [pr for name, pr in (("lh", (Xl, Wh)), ("hl", (Xh, Wl)), ("hh", (Xh, Wh))) if name != drop]
    pairs = [(a.t().contiguous(), b.t().contiguous()) for a, b in pairs]        # [K, rows]: a[k] is one column
    acc = torch.zeros(len(rows), p.N)
    part, tmp = torch.empty_like(acc), torch.empty_like(acc)
    for s in range(p.K // 64 - (1 if skip_last else 0)):
        for a, b in pairs:
            part.zero_()
            for k in range(64 * s, 64 * s + 64):
                torch.mul(a[k][:, None], b[k][None, :], out=tmp)
                part.add_(tmp)
            acc.add_(part)
    if epilogue:
        if q.bias is not None:
            acc = acc + torch.roll(q.bias, -bias_shift)[None, :]
        if q.res is not None:
            acc = acc + q.res[rows]
    return acc
