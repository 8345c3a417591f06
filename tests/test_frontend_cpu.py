"""CPU: the fp64 restatements of the step's front end (tests/frontend_ref.py) checked without a GPU -- against the oracle and
torch.nn.functional.normalize -- and the numbers the GPU tests (tests/test_frontend_gpu.py) rely on: the fp32 twin's error on
the inputs of every GPU case (the stored bars are held to it) and the conditions those inputs have to meet."""
import functools

import numpy as np
import torch

import frontend_ref as R
import nr_oracle as O

F32 = torch.float32
TINY = float(np.finfo(np.float32).tiny)


# ---- the references are right -----------------------------------------------------------------------------------------------
def test_prepare_equals_functional_normalize():
    q = R.make_tokens(17, 256)
    y, nrm, cs = R.prepare(q.x, q.mask)
    xn = torch.nn.functional.normalize(q.x.double(), dim=-1)
    assert float((y - xn * q.mask.double()[:, None]).abs().max()) <= 1e-12
    assert float((cs - xn.sum(0)).abs().max()) <= 1e-12                                   # UNMASKED rows: padding tokens count
    assert float((cs - y.sum(0)).abs().max()) > 1e-2                                      # ... and that is not the masked sum
    assert float(nrm[q.zero]) == 1e-12 and float(nrm[q.clamp]) == 1e-12
    assert float(y[q.zero].abs().max()) == 0.0
    assert abs(float(y[q.clamp].norm()) - 1e-2) <= 1e-9                                   # 1e-14 / 1e-12, not renormalised
    y0, nrm0, cs0 = R.prepare(q.x, q.mask, False)
    assert torch.equal(y0, q.x.double() * q.mask.double()[:, None]) and torch.equal(nrm0, nrm)
    assert float((cs0 - q.x.double().sum(0)).abs().max()) <= 1e-12
    y1, _, _ = R.prepare(q.x, None)
    assert float((y1 - xn).abs().max()) <= 1e-12


def test_split_is_round_to_nearest_even_and_the_remainder():
    v = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, 1.0 + 2.0 ** -8 + 2.0 ** -23])
    hi, lo = R.split(v)
    assert R.bf(hi).tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 0.0, 0.0, 1 + 2.0 ** -7]    # ties to even; above a tie: up
    assert int(hi[5]) == -32768 and int(hi[4]) == 0                                       # the sign of zero is kept
    x = R.make_split(257)
    hi, lo = R.split(x)
    assert float(((R.bf(hi) + R.bf(lo)) - x.double()).abs().div(x.double().abs().clamp_min(1e-300)).max()) <= 2.0 ** -17
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) >= 1e30


def test_centrality_equals_the_oracle_from_raw_features():
    """One global token per sample: R.chain (R.prepare's normalisation, the mean over ALL tokens, R.centrality) is
    O.centrality_weights to 1e-12; with G tokens the "mean" reduction is the oracle's too."""
    for B, Nt, Nv in R.CHAIN:
        q = R.make_chain(B, Nt, Nv)
        wt, wv = R.chain(q, R.CW_SCALE)
        ot, ov = O.centrality_weights(q.text.double(), q.video.double(), q.gt.double(), q.gv.double(), R.CW_SCALE)
        assert float((wt - ot).abs().max()) <= 1e-12 and float((wv - ov).abs().max()) <= 1e-12
        _, _, cs = R.prepare(q.text.reshape(-1, 512), q.tm.reshape(-1).float())
        w2, _, _ = R.centrality(q.gt, cs / (B * Nt), R.CW_SCALE)
        assert float((w2 - ot).abs().max()) <= 1e-12
    B, d = 5, 64
    x = torch.from_numpy(R._normal("cpu/x", (B, 7, d)))
    g3, g6 = torch.from_numpy(R._normal("cpu/g3", (B, 3, d))), torch.from_numpy(R._normal("cpu/g6", (B, 6, d)))
    ot, ov = O.centrality_weights(x, x, g3, g6, R.CW_SCALE, multi_token="mean")
    mean = torch.nn.functional.normalize(x.reshape(-1, d), dim=-1).mean(0)
    for g, o in ((g3, ot), (g6, ov)):
        w, gn, wtok = R.centrality(g, mean, R.CW_SCALE)
        assert float((w - o).abs().max()) <= 1e-12 and wtok.shape == gn.shape == g.shape[:2]
        assert float((gn - g.norm(dim=-1)).abs().max()) <= 1e-12


def test_normalize_bwd_equals_the_closed_form():
    """(g - xn <g, xn>) / ||x|| with g = mask d_xn + dmean / n_tok, row by row; g / 1e-12 on the zero row."""
    q = R.make_nbwd(5, 100)
    x, m = q.x.double(), q.mask.double()
    for d_xn, dmean in ((q.d_xn, None), (None, q.dmean), (q.d_xn, q.dmean)):
        got = R.normalize_bwd(q.x, q.mask, d_xn, dmean)
        g = (0 if d_xn is None else m[:, None] * d_xn.double()) + (0 if dmean is None else dmean.double()[None, :] / 5)
        g = g + torch.zeros_like(x)
        nrm = x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        xn = x / nrm
        want = (g - xn * (g * xn).sum(-1, keepdim=True)) / nrm
        assert R.row_rel_err(got, want) <= 1e-12
        assert float((got[1] - g[1] / 1e-12).abs().max()) <= 1e-12 * float(got[1].abs().max())
        if dmean is None:
            assert float(got[0].abs().max()) == 0.0                                       # the masked row: only dmean survives


def test_sums_and_bounds():
    a, b = R.make_gemm(5, 9, 48)
    assert float((R.gemm_nt(a, b) - torch.einsum("mk,nk->mn", a.double(), b.double())).abs().max()) <= 1e-12
    p = R.make_sum(13, 65)
    assert float((R.reduce_parts(p, 0.25) - 0.25 * p.double().sum(0)).abs().max()) <= 1e-12
    # a sequential fp32 sum -- the worst order there is -- stays inside the bounds
    s = torch.zeros(65)
    for r in range(13):
        s = s + p[r]
    sc = R.f32(R.SUM_SCALE)
    assert bool(((s * sc).double() - R.reduce_parts(p, sc)).abs().le(R.sum_bound(p, sc)).all())
    c = torch.zeros(5, 9)
    for k in range(48):
        c = c + a[:, k:k + 1] * b[:, k][None, :]
    assert bool((c.double() - R.gemm_nt(a, b)).abs().le(R.gemm_bound(a, b)).all())


# ---- the bars are earned ----------------------------------------------------------------------------------------------------
def _prep_cases():
    for d in R.PREP_D:
        for n in R.PREP_NTOK:
            for v in ((0, 1, 2, 3) if n == 1 else (0,)):
                yield R.make_tokens(n, d, v), n, d
    yield R.make_tokens(*R.PREP_BIG), R.PREP_BIG[0], R.PREP_BIG[1]
    yield R.make_tokens(*R.PREP_FLAG_SHAPE), R.PREP_FLAG_SHAPE[0], R.PREP_FLAG_SHAPE[1]
    for sa, sb in R.PAIR_SHAPES:
        for d in R.PAIR_D:
            for which, s in enumerate((sa, sb)):
                yield R.make_pair(s, d, which), s[0] * s[1], d


@functools.lru_cache(maxsize=None)
def _prepare_twin():
    e_y = {d: 0.0 for d in R.PREP_D}
    e_n = {d: 0.0 for d in R.PREP_D}
    e_c = {1: 0.0, 16: 0.0, 4096: 0.0}
    for q, n, d in _prep_cases():
        xn, nrm = R.normalize(q.x)
        xn32, nrm32 = R.normalize(q.x, F32)
        e_y[d] = max(e_y[d], float((xn32.double() - xn).abs().max()))
        above = nrm > 1e-12
        assert torch.equal(above, nrm32 > R.f32(1e-12))                       # the twin clamps the rows the reference clamps
        assert bool((nrm32[~above] == R.f32(1e-12)).all())
        if bool(above.any()):
            e_n[d] = max(e_n[d], float(((nrm32.double() - nrm)[above] / nrm[above]).abs().max()))
        if n <= 4097:
            k = R.bucket(n)
            e_c[k] = max(e_c[k], float((xn32.sum(0).double() - xn.sum(0)).abs().max()))
    return e_y, e_n, e_c


def _held(name, measured, stored, cap=None, bar=None):
    """The stored figure is the measured one rounded up (by less than a factor 2); FACTOR times it stays under the old bar."""
    print(f"twin {name}: measured {measured:.3g}, stored {stored:.3g}")
    assert 0.0 < measured <= stored, (name, measured, stored)
    assert measured >= 0.5 * stored, (name, measured, stored)
    if cap is not None:
        assert (R.FACTOR * stored if bar is None else bar) <= cap, (name, stored, cap)


def test_preparation_bars_are_eight_times_the_twin_and_under_the_old_bars():
    e_y, e_n, e_c = _prepare_twin()
    for d in R.PREP_D:
        # |ref| <= 1: the largest bar on hi + lo is 2^-17 + FACTOR E32_Y, on hi 2^-8 + 1.01 FACTOR E32_Y
        _held(f"y d={d}", e_y[d], R.E32_Y[d], R.CAP_HILO, 2.0 ** -17 + R.FACTOR * R.E32_Y[d])
        assert 2.0 ** -8 + 1.01 * R.FACTOR * R.E32_Y[d] <= R.CAP_HI
        _held(f"norm d={d}", e_n[d], R.E32_NORM[d], R.CAP_NORM)
    for k in e_c:
        _held(f"colsum n_tok~{k}", e_c[k], R.E32_COLSUM[k], R.CAP_COLSUM)
    assert R.FACTOR == 8.0


def test_gemm_bars():
    """FRAC_GEMM[K] = the share of the rigorous bound the twin uses (max over the cases with that K and over entries); the bar
    of an entry is min(1, 8 FRAC) of the bound, and never above the old 2e-5 max|ref|."""
    cases = [(M, N, K) for M, N in R.GEMM_MN for K in R.GEMM_K] + [R.GEMM_PREFILTER]
    frac = {}
    for M, N, K in cases:
        a, b = R.make_gemm(M, N, K)
        ref, bound = R.gemm_nt(a, b), R.gemm_bound(a, b)
        frac[K] = max(frac.get(K, 0.0), float(((R.gemm_nt(a, b, F32).double() - ref).abs() / bound).max()))
        if M * N >= 100:                                     # (a single entry can be a cancellation remainder: no max|ref| there)
            assert float((min(1.0, R.FACTOR * R.FRAC_GEMM[K]) * bound).max()) <= R.CAP_GEMM * float(ref.abs().max()), (M, N, K)
    for K, f in sorted(frac.items()):
        _held(f"gemm K={K}", f, R.FRAC_GEMM[K])
    assert frac[16] > 0.1 and frac[1024] < 0.005                       # few terms: the bound itself; many: far inside it


def _cw_cases():
    for B in R.CWP_B:
        for G in sorted({g for pair in R.CWP_G for g in pair}):
            for d in R.CWP_D:
                for side in "tv":
                    yield R.make_cw(B, G, d, side)
    for d in R.CWS_D:
        for n_parts in R.CWS_PARTS:
            n_tok = 16 * n_parts
            parts = R.make_cw_parts(n_parts, n_tok, d, "single")
            for B in R.CWS_B:
                g = R.make_cw_single(B, d, parts, n_tok, "single")
                yield g[:, None, :], parts.double().sum(0) * R.f32(1.0 / n_tok)


def test_centrality_bars_and_conditions():
    e_w = e_g = 0.0
    lo, hi = 1.0, -1.0
    for g, mean in _cw_cases():
        w, gn, wtok = R.centrality(g, mean, R.CW_SCALE)
        w32, gn32, wtok32 = R.centrality(g, mean.float(), R.CW_SCALE, F32)
        arg = torch.log(wtok)
        assert float(arg.abs().max()) < 1.0                                                # |scale * cos| < 1
        lo, hi = min(lo, float(arg.min())), max(hi, float(arg.max()))
        z = gn == 1e-12
        assert int(z.sum()) == 1 and bool((wtok[z] == 1.0).all()) and bool((wtok32[z] == 1.0).all())      # the zero token
        e_w = max(e_w, float((w32.double() - w).abs().max()), float((wtok32.double() - wtok).abs().max()))
        e_g = max(e_g, float(((gn32.double() - gn) / gn)[~z].abs().max()) if bool((~z).any()) else 0.0)
    assert lo < -0.15 and hi > 0.01, (lo, hi)                                              # cosines of size, both signs
    _held("centrality w", e_w, R.E32_CW, R.CAP_CW)
    _held("centrality gnorm", e_g, R.E32_GNORM, R.CAP_NORM)
    e = 0.0
    for B, Nt, Nv in R.CHAIN:
        q = R.make_chain(B, Nt, Nv)
        for a, b in zip(R.chain(q, R.CW_SCALE), R.chain(q, R.CW_SCALE, F32)):
            e = max(e, float((b.double() - a).abs().max()))
    _held("centrality chain", e, R.E32_CW_CHAIN, R.CAP_CW)


def test_normalize_bwd_bar():
    e = 0.0
    for n in R.NBWD_NTOK:
        for d in R.NBWD_D:
            q = R.make_nbwd(n, d)
            nrm = q.x.double().norm(dim=-1)
            assert bool(((nrm == 0) | (nrm > 1.0)).all())                                  # no row inside (0, 1e-12): out of scope
            for mask in (q.mask, None):
                for d_xn, dmean in ((q.d_xn, None), (None, q.dmean), (q.d_xn, q.dmean)):
                    ref = R.normalize_bwd(q.x, mask, d_xn, dmean)
                    e = max(e, R.row_rel_err(R.normalize_bwd(q.x, mask, d_xn, dmean, F32), ref))
    _held("normalize_bwd", e, R.E32_NBWD, R.CAP_NBWD)


# ---- the inputs are what the GPU tests say they are ---------------------------------------------------------------------------
def _no_subnormal(t):
    a = t.double().abs()
    return bool(((a == 0) | (a >= TINY)).all())


def test_input_conditions():
    for q, n, d in _prep_cases():
        assert _no_subnormal(q.x), (n, d)
        if getattr(q, "clamp", None) is not None:
            r = q.x[q.clamp].double()
            assert abs(float(r.norm()) - 1e-14) <= 1e-20
            assert float((r * r).min()) >= TINY and float((q.x[q.clamp] * q.x[q.clamp]).min()) >= TINY     # normal squares, in fp32 too
            assert float(q.x[q.clamp].norm()) < R.f32(1e-12)
            assert float(q.mask[q.clamp]) == 1.0 and float(q.mask[q.zero]) == 1.0
        if n >= 12 and hasattr(q, "zero"):
            assert float(q.x[q.zero].abs().max()) == 0.0
            m = q.mask.tolist()
            assert m[8:12] == [0.0] * 4 and 0.0 < sum(m) < n                              # a fully masked sample, ragged elsewhere
            assert len({sum(m[i:i + 4]) for i in range(0, min(n, 64) // 4 * 4, 4)}) > 1
    for n in R.SPLIT_N:
        x = R.make_split(n)
        assert _no_subnormal(x) and bool(torch.isfinite(x).all())
    for M, N, K in [(37, 50, 1024), R.GEMM_PREFILTER]:
        assert all(_no_subnormal(t) for t in R.make_gemm(M, N, K))
    for g, mean in _cw_cases():
        assert _no_subnormal(g) and _no_subnormal(mean.float())
    # the part-count edges the token counts are there for (nr_prepare_parts: 16 tokens per part up to 256 parts)
    parts = lambda n: min(max((n + 15) // 16, 1), 256)
    assert [parts(n) for n in R.PREP_NTOK] == [1, 1, 1, 2, 256, 256]
    assert (4097 - 1) // (256 * 4) == 4 and (4096 - 1) // (256 * 4) == 3                  # a fifth row for one wave at 4097 only
    assert R.PREP_BIG[0] > 2048 * 16 and R.PREP_BIG[0] * R.PREP_BIG[1] * 4 < 35e6
