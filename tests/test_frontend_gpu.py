"""GPU: every launch form of the step's front end against the fp64 restatements of tests/frontend_ref.py.

  (a) nr_prepare_tokens: every width, the part boundary, the 256-part cap, the 2048-workgroup cap, every flag combination
  (b) nr_prepare_tokens_pair: bit for bit the two single launches, the mixed forms included
  (c) nr_split_bf16: bit for bit torch's round-to-nearest-even conversion and its remainder
  (d) nr_gemm_nt_f32: idle K-splitting waves, the in-loop k < K guard, ragged last trips, clamped operand rows
  (e) nr_reduce_parts and nr_colsum_group (ops.colsum_pair): every tail of their unrolled loops
  (f) nr_centrality_weights_pair / nr_centrality_weights: several global tokens, per-token outputs, part-count edges, the chain
      the step runs from raw features against the oracle
  (g) nr_normalize_bwd against fp64 autograd

The bars are frontend_ref's: FACTOR = 8 times the error of the same formulas in plain fp32 on the CPU on exactly these inputs
(measured and re-asserted by tests/test_frontend_cpu.py, never taken from a kernel), plus the exact bf16 terms; pure sums are held
to the rounding bound that holds for any order.  Every figure is printed before it is asserted."""
import functools
from types import SimpleNamespace

import pytest
import torch

import frontend_ref as R
import nr_oracle as O
from neighborretr_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x5A5A                                   # int16 sentinel; 0x5A5A5A5A as fp32 is 1.5e16
F32_EPS = R.f32(1e-12)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _is_zero(bits):
    """bf16 bit patterns that are +0 or -0."""
    return (bits.cpu().to(torch.int32) & 0x7FFF) == 0


# ---- (a) preparation, single launch -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _tokens(n_tok, d, variant=0):
    """(inputs on the CPU, x and mask on the device) -- made once, shared, never written to."""
    q = R.make_tokens(n_tok, d, variant)
    return q, _dev(q.x), _dev(q.mask)


def _raw_prepare(x, mask, normalize, lo=True, norm=True, colsum=True):
    """nr_prepare_tokens through hip.call with all four outputs inside ONE allocation filled with a sentinel, 64 elements of
    guard around each: whatever was not asked for, and every guard, must still hold the sentinel afterwards."""
    n, d = x.shape
    parts = hip.prepare_parts(n)
    want = dict(hi=True, lo=lo, norm=norm, colsum=colsum)
    where, off = {}, 64
    for name, size in (("hi", n * d), ("lo", n * d), ("norm", 2 * n), ("colsum", 2 * parts * d)):        # in int16 elements
        where[name] = (off, off + size)
        off += (size + 63) // 64 * 64 + 64
    arena = torch.full((off,), SENT, dtype=torch.int16, device=DEV)
    view = lambda k: arena[where[k][0]:where[k][1]]
    p = lambda k: hip.ptr(view(k)) if want[k] else None
    hip.call("nr_prepare_tokens", hip.ptr(x), hip.ptr(mask, allow_none=True), n, d, int(normalize), p("hi"), p("lo"), p("norm"),
             p("colsum"), hip.stream_ptr())
    torch.cuda.synchronize()
    untouched = torch.ones(off, dtype=torch.bool, device=DEV)
    for k, (a, b) in where.items():
        if want[k]:
            untouched[a:b] = False
    assert bool((arena[untouched] == SENT).all()), "a launch wrote outside the outputs it was given"
    return SimpleNamespace(hi=view("hi").view(n, d), lo=view("lo").view(n, d) if lo else None,
                           norm=view("norm").view(torch.float32) if norm else None,
                           colsum=view("colsum").view(torch.float32).view(parts, d) if colsum else None)


def _check_prepared(tag, q, out, normalize=True, masked=True):
    """Every assertion of the single launch that the outputs present allow.  out: hi, lo, norm, colsum (None: not asked for)."""
    n, d = q.x.shape
    mask = q.mask if masked else None
    y, nrm, cs = R.prepare(q.x, mask, normalize)
    e_y = R.FACTOR * R.E32_Y[d] if normalize else 0.0                     # normalize = 0: x * mask is exact in fp32
    zero_rows = torch.zeros(n, dtype=torch.bool) if mask is None else mask == 0
    if q.zero is not None:
        zero_rows[q.zero] = True
    hi = R.bf(out.hi)
    r = float(((hi - y).abs() / (2.0 ** -8 * y.abs() + 1.01 * e_y + 1e-300)).max())
    print(f"frontend {tag}: hi {float((hi - y).abs().max()):.2e}, {r:.3f} of its bar")
    assert r <= 1.0
    assert bool(_is_zero(out.hi)[zero_rows].all())
    if out.lo is not None:
        both = hi + R.bf(out.lo)
        r = float(((both - y).abs() / (2.0 ** -17 * y.abs() + e_y + 1e-300)).max())
        print(f"frontend {tag}: hi + lo {float((both - y).abs().max()):.2e}, {r:.3f} of its bar")
        assert r <= 1.0
        assert bool(_is_zero(out.lo)[zero_rows].all())
    if out.norm is not None:
        got = out.norm.cpu().double()
        clamped = nrm == 1e-12
        assert bool((out.norm.cpu()[clamped] == F32_EPS).all())           # the zero row and the 1e-14 row: float32(1e-12) exactly
        for k in (q.zero, q.clamp):
            assert k is None or bool(clamped[k])
        if bool((~clamped).any()):
            r = float(((got - nrm) / nrm)[~clamped].abs().max())
            print(f"frontend {tag}: norm {r:.2e} relative (bar {R.FACTOR * R.E32_NORM[d]:.1e})")
            assert r <= R.FACTOR * R.E32_NORM[d]
    if out.colsum is not None:
        assert out.colsum.shape == (hip.prepare_parts(n), d)
        got = out.colsum.cpu().double().sum(0)                            # the sum only, not which rows a part holds
        src = R.normalize(q.x)[0] if normalize else q.x.double()
        bound = R.sum_bound(src, 1.0)
        if normalize:
            bound = torch.minimum(bound + n * e_y, torch.full_like(bound, R.FACTOR * R.E32_COLSUM[R.bucket(n)]))
        r = float(((got - cs).abs() / bound.clamp_min(1e-300)).max())
        print(f"frontend {tag}: colsum {float((got - cs).abs().max()):.2e}, {r:.3f} of its bar")
        assert r <= 1.0


@pytest.mark.parametrize("n_tok", R.PREP_NTOK)
@pytest.mark.parametrize("d", R.PREP_D)
def test_prepare_single_with_column_sums(d, n_tok):
    """ops.prepare_tokens as the callers use it, every output on.  n_tok = 1: three waves of the only workgroup have no row and
    their partial column sums must be zero -- run with the one row ordinary, exactly zero, under the clamp, and masked."""
    for variant in ((0, 1, 2, 3) if n_tok == 1 else (0,)):
        q, x, mask = _tokens(n_tok, d, variant)
        prep = ops.prepare_tokens(x, mask, want_colsum=True)
        _check_prepared(f"prepare d={d} n_tok={n_tok} v{variant}", q, prep)


def test_prepare_past_the_grid_cap_without_column_sums():
    """The memory-bank form: 32773 tokens on 2048 workgroups; one trip of the batched-load loop covers 2048 * 16 rows, the last 5
    rows are five waves' second trip."""
    n_tok, d = R.PREP_BIG
    q, x, mask = _tokens(n_tok, d)
    prep = ops.prepare_tokens(x, mask)
    assert prep.colsum is None
    _check_prepared(f"prepare d={d} n_tok={n_tok} bank form", q, prep)


FLAGS = [dict(masked=False), dict(normalize=0), dict(lo=False), dict(norm=False), dict(lo=False, norm=False),
         dict(colsum=False), dict(normalize=0, masked=False, lo=False), dict()]


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "-".join(f"{k}={int(v)}" for k, v in f.items()) or "all")
def test_prepare_flag_combinations(flags):
    """mask = None; normalize = 0 (hi + lo is the raw masked x to 2^-17, norm still the clamped norm, column sums of raw x);
    lo = NULL (the evaluator's bf16 plan); norm = NULL; column sums alone; and what was not asked for is not written."""
    n_tok, d = R.PREP_FLAG_SHAPE
    q, x, mask = _tokens(n_tok, d)
    f = dict(flags)
    masked, normalize = f.pop("masked", True), f.pop("normalize", 1)
    out = _raw_prepare(x, mask if masked else None, normalize, **f)
    _check_prepared(f"prepare flags {flags}", q, out, bool(normalize), masked)
    if not flags:                                                         # ops.prepare_tokens is the same launch
        prep = ops.prepare_tokens(x, mask, want_colsum=True)
        assert all(torch.equal(getattr(prep, k), getattr(out, k)) for k in ("hi", "lo", "norm", "colsum"))
    if flags == dict(lo=False):
        prep = ops.prepare_tokens(x, mask, want_lo=False, want_colsum=True)
        assert prep.lo is None and torch.equal(prep.hi, out.hi) and torch.equal(prep.colsum, out.colsum)


def test_prepare_refusals():
    hi = torch.zeros(4 * 1280, dtype=torch.int16, device=DEV)
    x = torch.ones(4 * 1280, device=DEV)
    for n_tok, d in ((4, 128), (4, 1280), (0, 256)):
        with pytest.raises(hip.NrHipError):
            hip.call("nr_prepare_tokens", hip.ptr(x), None, n_tok, d, 1, hip.ptr(hi), None, None, None, hip.stream_ptr())
        with pytest.raises(hip.NrHipError):
            hip.call("nr_prepare_tokens_pair", hip.ptr(x), None, n_tok, hip.ptr(hi), None, None, None,
                     hip.ptr(x), None, 4, hip.ptr(hi), None, None, None, d, 1, hip.stream_ptr())
    torch.cuda.synchronize()
    assert float(hi.abs().max()) == 0.0


# ---- (b) preparation, pair launch ---------------------------------------------------------------------------------------------
def _launch(specs, normalize):
    """One launch for one spec (nr_prepare_tokens) or two (nr_prepare_tokens_pair); spec = (x, mask or None, lo, norm, colsum).
    -> per spec a dict of the planes asked for."""
    outs, argv = [], []
    for x, mask, lo, norm, colsum in specs:
        n, d = x.shape
        o = dict(hi=torch.full((n, d), SENT, dtype=torch.int16, device=DEV))
        if lo:
            o["lo"] = torch.full((n, d), SENT, dtype=torch.int16, device=DEV)
        if norm:
            o["norm"] = torch.full((n,), -7.0, device=DEV)
        if colsum:
            o["colsum"] = torch.full((hip.prepare_parts(n), d), -7.0, device=DEV)
        outs.append(o)
        g = lambda k: hip.ptr(o[k]) if k in o else None
        argv.append((hip.ptr(x), hip.ptr(mask, allow_none=True), n, g("hi"), g("lo"), g("norm"), g("colsum")))
    d = specs[0][0].shape[1]
    if len(specs) == 1:
        a = argv[0]
        hip.call("nr_prepare_tokens", a[0], a[1], a[2], d, normalize, *a[3:], hip.stream_ptr())
    else:
        hip.call("nr_prepare_tokens_pair", *argv[0], *argv[1], d, normalize, hip.stream_ptr())
    torch.cuda.synchronize()
    return outs


PAIR_FORMS = [                                  # ((lo, norm, colsum, masked) of the first tensor, the same of the second, normalize)
    ((True, True, True, True), (True, True, True, True), 1),
    ((True, True, True, True), (True, True, False, True), 1),            # column sums on one side only
    ((True, True, False, True), (True, True, True, True), 1),
    ((True, True, True, True), (True, True, True, False), 1),            # a mask on one side only
    ((True, True, True, False), (False, False, True, True), 1),
    ((True, True, True, True), (True, True, True, True), 0),             # normalize = 0
    ((False, True, False, True), (True, False, True, False), 0),
]


@pytest.mark.parametrize("d", R.PAIR_D)
@pytest.mark.parametrize("shapes", R.PAIR_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}+{s[1][0]}x{s[1][1]}")
def test_prepare_pair_is_bit_for_bit_the_two_single_launches(shapes, d):
    """csrc/nr_prepare.hip promises unchanged arithmetic and order: the part count and the workgroup-to-row map of a tensor are
    the same functions in both launches, so every plane -- the column-sum PARTS included -- has the single launch's bits.  (The
    single launch is held to fp64 by the tests above.)"""
    q = [R.make_pair(s, d, k) for k, s in enumerate(shapes)]
    x = [_dev(t.x) for t in q]
    m = [_dev(t.mask) for t in q]
    for fa, fb, normalize in PAIR_FORMS:
        specs = [(x[k], m[k] if f[3] else None, f[0], f[1], f[2]) for k, f in enumerate((fa, fb))]
        pair = _launch(specs, normalize)
        for k in (0, 1):
            single = _launch([specs[k]], normalize)[0]
            assert single.keys() == pair[k].keys()
            for name in single:
                assert torch.equal(single[name], pair[k][name]), (fa, fb, normalize, k, name)
    # through ops.prepare_tokens_pair, with and without the column sums and lo
    for want_lo in (True, False):
        for want_colsum in (True, False):
            pa, pb = ops.prepare_tokens_pair(x[0], m[0], x[1], m[1], want_lo=want_lo, want_colsum=want_colsum)
            for k, p in enumerate((pa, pb)):
                s = ops.prepare_tokens(x[k], m[k], want_lo=want_lo, want_colsum=want_colsum)
                assert (p.lo is None) == (not want_lo) and (p.colsum is None) == (not want_colsum)
                for name in ("hi", "lo", "norm", "colsum"):
                    a, b = getattr(p, name), getattr(s, name)
                    assert (a is None and b is None) or torch.equal(a, b), (want_lo, want_colsum, k, name)
                if want_lo and want_colsum:
                    _check_prepared(f"pair {shapes} d={d} tensor {k}", SimpleNamespace(x=q[k].x, mask=q[k].mask, zero=None, clamp=None), p)


# ---- (c) nr_split_bf16 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SPLIT_N)
def test_split_bf16_is_round_to_nearest_even_bit_for_bit(n):
    """Lengths around the 256-thread block and past the 2048-block cap (a second stride for three elements); exact ties, +-0,
    magnitudes from 1e-30 to 1e30.  Subnormals, infinities and NaN are LEFT OUT: the hardware conversion's behaviour on
    subnormals has not been measured and no caller feeds any of them."""
    x = R.make_split(n)
    want_hi, want_lo = R.split(x)
    hi, lo = ops.split_bf16(x.to(DEV))
    assert torch.equal(hi.cpu(), want_hi) and torch.equal(lo.cpu(), want_lo)
    arena = torch.full((n + 128,), SENT, dtype=torch.int16, device=DEV)        # lo = NULL, and nothing written past the end
    hip.call("nr_split_bf16", hip.ptr(x.to(DEV)), n, hip.ptr(arena[64:64 + n]), None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(arena[64:64 + n].cpu(), want_hi)
    assert bool((arena[:64] == SENT).all()) and bool((arena[64 + n:] == SENT).all())
    hi2, lo2 = ops.split_bf16(x.to(DEV), want_lo=False)
    assert lo2 is None and torch.equal(hi2, hi)


# ---- (d) nr_gemm_nt_f32 -------------------------------------------------------------------------------------------------------
def _gemm_case(M, N, K):
    a, b = R.make_gemm(M, N, K)
    c = ops.gemm_nt_f32(a.to(DEV), b.to(DEV))
    assert c.shape == (M, N)
    bar = min(1.0, R.FACTOR * R.FRAC_GEMM[K]) * R.gemm_bound(a, b)
    err = (c.cpu().double() - R.gemm_nt(a, b)).abs()
    return float((err / bar).max()), float(err.max())


@pytest.mark.parametrize("K", R.GEMM_K)
def test_gemm_nt_f32_against_fp64(K):
    """K = 16: three of the four K-splitting waves idle; 48, 240, 272: the in-loop k < K guard; 272, 1024: second trips, the
    first of them ragged; M = 1 / N = 1: every lane of the tile reads the clamped row."""
    worst = 0.0
    for M, N in R.GEMM_MN:
        r, e = _gemm_case(M, N, K)
        print(f"frontend gemm {M}x{N}x{K}: max|d| {e:.2e}, {r:.3f} of its bar")
        worst = max(worst, r)
    print(f"frontend gemm K={K}: worst ratio to the bar {worst:.3f}")
    assert worst <= 1.0


def test_gemm_nt_f32_prefilter_shape_and_refusal():
    M, N, K = R.GEMM_PREFILTER
    r, e = _gemm_case(M, N, K)
    print(f"frontend gemm {M}x{N}x{K}: max|d| {e:.2e}, {r:.3f} of its bar")
    assert r <= 1.0
    a, b = (t.to(DEV) for t in R.make_gemm(3, 5, 24))
    with pytest.raises(hip.NrHipError):                                   # K % 16 != 0
        ops.gemm_nt_f32(a, b)


# ---- (e) partial-sum reductions -----------------------------------------------------------------------------------------------
def test_reduce_parts_at_every_tail():
    """nr_reduce_parts: wave w takes parts w, w + 4, ... four at a time; n_parts = 13 (mod 16) is the last count its tail loop
    handles alone, 16 k + 1 the first after a full unrolled trip.  n = 63 / 64 / 65 columns: the last workgroup's lanes."""
    scale = R.f32(R.SUM_SCALE)
    worst = 0.0
    for n_parts in R.SUM_ROWS:
        for n in R.SUM_COLS:
            p = R.make_sum(n_parts, n)
            got = ops.reduce_parts(p.to(DEV), scale).cpu().double()
            r = float(((got - R.reduce_parts(p, scale)).abs() / R.sum_bound(p, scale)).max())
            worst = max(worst, r)
            assert r <= 1.0, (n_parts, n, r)
    print(f"frontend reduce_parts: worst ratio to the rounding bound {worst:.3f}")


def test_colsum_pair_at_every_tail():
    """nr_colsum_group as ops.colsum_pair launches it: two items of DIFFERENT shapes in one grid; wave w of 16 takes rows w,
    w + 16, ... four at a time: rows = 49 (mod 64) is its tail's edge."""
    sa, sb = R.f32(R.SUM_SCALE), R.f32(0.375)
    worst = 0.0
    shapes = [(r, c) for r in R.SUM_ROWS for c in R.SUM_COLS]
    for k, (rows, cols) in enumerate(shapes):
        rows_b, cols_b = shapes[(k * 7 + 11) % len(shapes)]               # 7 and 70 are coprime: every shape is the second item once
        a, b = R.make_sum(rows, cols), R.make_sum(rows_b, cols_b, "sum_b")
        oa, ob = ops.colsum_pair(a.to(DEV), sa, b.to(DEV), sb)
        for got, src, sc in ((oa, a, sa), (ob, b, sb)):
            assert got.shape == (src.shape[1],)
            r = float(((got.cpu().double() - R.colsum(src, sc)).abs() / R.sum_bound(src, sc)).max())
            worst = max(worst, r)
            assert r <= 1.0, (rows, cols, rows_b, cols_b, r)
    print(f"frontend colsum_pair: worst ratio to the rounding bound {worst:.3f}")


# ---- (f) centrality weights ---------------------------------------------------------------------------------------------------
def _check_cw(tag, g, mean, w, gnorm, wtok=None):
    """w [B], gnorm [B * G], wtok [B * G] or None of one side against fp64; the all-zero token has norm float32(1e-12), weight 1."""
    B, G, _ = g.shape
    w_ref, gn_ref, wtok_ref = R.centrality(g, mean, R.CW_SCALE)
    e = [float((w.cpu().double() - w_ref).abs().max())]
    zero = (gn_ref == 1e-12).reshape(-1)
    assert int(zero.sum()) == 1
    if G == 1:
        assert bool((w.cpu()[zero] == 1.0).all())
    assert gnorm.shape == (B * G,) and bool((gnorm.cpu()[zero] == F32_EPS).all())          # [i * G + t]
    rn = float(((gnorm.cpu().double() - gn_ref.reshape(-1)) / gn_ref.reshape(-1))[~zero].abs().max()) if B * G > 1 else 0.0
    assert rn <= R.FACTOR * R.E32_GNORM, (tag, rn)
    if wtok is not None:
        assert wtok.shape == (B * G,) and bool((wtok.cpu()[zero] == 1.0).all())
        e.append(float((wtok.cpu().double() - wtok_ref.reshape(-1)).abs().max()))
    assert max(e) <= R.FACTOR * R.E32_CW, (tag, e)
    return max(e)


@pytest.mark.parametrize("d", R.CWP_D)
@pytest.mark.parametrize("Gt,Gv", R.CWP_G)
def test_centrality_weights_pair_against_fp64(Gt, Gv, d):
    """The production form: one wave per (sample, modality) walking the sample's global tokens ("mean" reduction), per-token
    norms and weights at [i * G + t].  B = 1 .. 16: the last workgroup is partial unless B % 4 == 0.  d = 68: any multiple of 4."""
    worst = 0.0
    for B in R.CWP_B:
        (gt, mt), (gv, mv) = R.make_cw(B, Gt, d, "t"), R.make_cw(B, Gv, d, "v")
        dgt, dgv, dmt, dmv = (_dev(t) for t in (gt, gv, mt, mv))
        w_t, w_v, aux = ops.centrality_weights_pair(dgt, dgv, dmt, dmv, R.CW_SCALE, want_aux=True)
        worst = max(worst, _check_cw(f"text B={B}", gt, mt, w_t, aux[0], aux[2]), _check_cw(f"video B={B}", gv, mv, w_v, aux[1], aux[3]))
        w_t2, w_v2, none = ops.centrality_weights_pair(dgt, dgv, dmt, dmv, R.CW_SCALE)
        assert none is None and torch.equal(w_t, w_t2) and torch.equal(w_v, w_v2)
        if Gt == Gv == 1:                                                 # a 2-D g is the [B, 1, d] call
            w_t3, w_v3, aux3 = ops.centrality_weights_pair(dgt[:, 0], dgv[:, 0], dmt, dmv, R.CW_SCALE, want_aux=True)
            assert torch.equal(w_t, w_t3) and torch.equal(w_v, w_v3) and all(torch.equal(a, b) for a, b in zip(aux, aux3))
    print(f"frontend centrality pair G=({Gt},{Gv}) d={d}: worst |d| {worst:.2e} (bar {R.FACTOR * R.E32_CW:.1e})")


@pytest.mark.parametrize("d", R.CWS_D)
def test_centrality_weights_single_against_fp64_and_the_pair_form(d):
    """nr_centrality_weights: 8 samples per workgroup (B = 7 / 8 / 9 / 17), the second column pass (d > 512), the mean rebuilt
    from 1 .. 256 parts (4 waves x 4 parts in flight: 3 / 4 / 5 / 17 are its edges).  The pair form on the mean this launch
    wrote agrees within the bar (not bit for bit: the two reduce in different orders)."""
    worst = worst_mean = 0.0
    for n_parts in R.CWS_PARTS:
        n_tok = 16 * n_parts
        parts = R.make_cw_parts(n_parts, n_tok, d, "single")
        inv = R.f32(1.0 / n_tok)
        mean_ref = R.reduce_parts(parts, inv)
        for B in R.CWS_B:
            g = R.make_cw_single(B, d, parts, n_tok, "single")
            dg = _dev(g)
            w, gnorm, mean = ops.centrality_weights(dg, _dev(parts), n_tok, R.CW_SCALE, want_aux=True)
            r = float(((mean.cpu().double() - mean_ref).abs() / R.sum_bound(parts, inv)).max())
            worst_mean = max(worst_mean, r)
            assert r <= 1.0, (n_parts, B, r)
            worst = max(worst, _check_cw(f"single B={B} parts={n_parts}", g[:, None, :], mean_ref, w, gnorm))
            w0, none, none2 = ops.centrality_weights(dg, _dev(parts), n_tok, R.CW_SCALE)
            assert none is None and none2 is None and torch.equal(w, w0)
            w_p, _, _ = ops.centrality_weights_pair(dg, dg, mean, mean, R.CW_SCALE)
            assert float((w_p - w).abs().max()) <= R.FACTOR * R.E32_CW
    print(f"frontend centrality single d={d}: worst |d| {worst:.2e} (bar {R.FACTOR * R.E32_CW:.1e}), mean {worst_mean:.3f} of its bound")


@pytest.mark.parametrize("B,Nt,Nv", R.CHAIN)
def test_the_steps_chain_from_raw_features_against_the_oracle(B, Nt, Nv):
    """prepare_tokens_pair(want_colsum) -> colsum_pair -> centrality_weights_pair, as head.py runs it, against
    O.centrality_weights on the raw features in fp64."""
    q = R.make_chain(B, Nt, Nv)
    pt, pv = ops.prepare_tokens_pair(_dev(q.text), _dev(q.tm), _dev(q.video), _dev(q.vm), want_colsum=True)
    mean_t, mean_v = ops.colsum_pair(pt.colsum, 1.0 / pt.n_tok, pv.colsum, 1.0 / pv.n_tok)
    w_t, w_v, _ = ops.centrality_weights_pair(_dev(q.gt), _dev(q.gv), mean_t, mean_v, R.CW_SCALE)
    ot, ov = O.centrality_weights(q.text.double(), q.video.double(), q.gt.double(), q.gv.double(), R.CW_SCALE)
    e = max(float((w_t.cpu().double() - ot).abs().max()), float((w_v.cpu().double() - ov).abs().max()))
    print(f"frontend centrality chain B={B}: |d| {e:.2e} (bar {R.FACTOR * R.E32_CW_CHAIN:.1e})")
    assert e <= R.FACTOR * R.E32_CW_CHAIN


def test_centrality_refusals():
    g = torch.ones(4, 1, 66, device=DEV)
    m = torch.ones(66, device=DEV)
    with pytest.raises(hip.NrHipError):                                   # d % 4 != 0
        ops.centrality_weights_pair(g, g, m, m, R.CW_SCALE)
    g, m, w = torch.ones(4, 1, 64, device=DEV), torch.ones(64, device=DEV), torch.zeros(4, device=DEV)
    for n_gt, n_gv in ((0, 1), (1, 0)):                                   # zero global tokens
        with pytest.raises(hip.NrHipError):
            hip.call("nr_centrality_weights_pair", hip.ptr(g), hip.ptr(g), 4, n_gt, n_gv, 64, hip.ptr(m), hip.ptr(m), R.CW_SCALE,
                     hip.ptr(w), hip.ptr(w), None, None, None, None, hip.stream_ptr())


# ---- (g) nr_normalize_bwd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.NBWD_D)
@pytest.mark.parametrize("n_tok", R.NBWD_NTOK)
def test_normalize_bwd_against_fp64_autograd(n_tok, d):
    """Row 0 is masked (only the dmean part survives), row 1 exactly zero (the clamp's g / 1e-12, from autograd and the kernel
    alike).  Rows with 0 < ||x|| < 1e-12 are OUT OF SCOPE and not generated: the kernel projects there, the clamp's derivative
    does not; neither is asserted."""
    q = R.make_nbwd(n_tok, d)
    x, mask, d_xn, dmean = (_dev(t) for t in (q.x, q.mask, q.d_xn, q.dmean))
    norm = ops.prepare_tokens(x).norm if d % 256 == 0 else x.norm(dim=-1).clamp_min(F32_EPS)
    worst = 0.0
    for m_dev, m_cpu in ((mask, q.mask), (None, None)):
        for use_xn, use_mean in ((True, False), (False, True), (True, True)):
            dx = ops.normalize_bwd(x, norm, m_dev, d_xn if use_xn else None, dmean if use_mean else None)
            ref = R.normalize_bwd(q.x, m_cpu, q.d_xn if use_xn else None, q.dmean if use_mean else None)
            assert dx.shape == (n_tok, d)
            r = R.row_rel_err(dx.cpu(), ref)
            worst = max(worst, r)
            assert r <= R.FACTOR * R.E32_NBWD, (m_cpu is not None, use_xn, use_mean, r)
            if m_cpu is not None and not use_mean:
                assert float(dx[0].abs().max()) == 0.0
    print(f"frontend normalize_bwd n_tok={n_tok} d={d}: worst row error {worst:.2e} (bar {R.FACTOR * R.E32_NBWD:.1e})")
