"""GPU: mutual proximity -- emp, gauss (neighborretr_amd/csrc/nr_mutualprox.hip, evaluator.sharded_mutual_proximity_*).

The count kernels against the restatement's integers (mutualprox_ref) on planted matrices (a grid of 1/32 with ties, signed zeros,
infinities, NaN, an all-NaN row and column) at the shapes where the kernels change path; accumulation over uneven blocks of
reference rows; the emp apply bit for bit; the moments to 1e-6 of fp64 and the gauss apply within 4 x the float32 restatement's own
distance from the fp64 formulas; the same bits of emp's T whatever the world size; the sharded evaluator under emulated ranks and
two gloo ranks, single- and multi-sentence, test-set and querybank lines; that both modes take a planted hub out of the lists;
eval_epoch and main_retrieval.py with and without the flag.

"The same bits" below means: NaN in the same places (a NaN's sign and payload are not part of the definition) and the same
bits everywhere else.

Measured on one MI355X (the figures the gauss tests print; DESIGN.md "Mutual proximity", Accuracy): gauss apply on the planted-hub
matrix, n = 96: GPU distance from the fp64 formulas 1.03e-6, bar 4.03e-6; n = 1000: 1.93e-6, bar 7.71e-6."""
import functools
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hubness_ref as H
import hubnorm_ref as R
import mutualprox_ref as MP
from neighborretr_amd import comm, evaluator, modeling, ops, synth, training
from util import golden, params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
N, Nt, Nv = 96, 24, 12
MODES = MP.MODES
ROW_CHUNK, ROW_TILE = 1024, 1024        # nr_mp_row_counts: floats of a reference row per LDS chunk; columns per workgroup
COL_TILE, COL_BLOCK = 16, 64            # nr_mp_col_counts: rows of S per wave (the register tile) and per workgroup


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _planted(n, L, seed, rare_inf=False):
    """Scores on a grid of 1/32 (ties abound) with signed zeros, infinities and NaN sprinkled in, a row of -inf, an all-NaN column, a
    column of signed zeros and an all-NaN row.  rare_inf: two infinities in all instead of 2.5 % (an infinity
    makes the moments of its two lines NaN)."""
    rng = np.random.default_rng(seed)
    S = (np.round(rng.standard_normal((n, L)) * 8) / 32).astype(np.float32)
    flat = S.reshape(-1)
    sprinkle = [(0.0, 0.05), (-0.0, 0.05), (np.nan, 0.05)] + ([] if rare_inf else [(np.inf, 0.005), (-np.inf, 0.02)])
    for val, frac in sprinkle:
        at = rng.choice(flat.size, max(1, int(frac * flat.size)), replace=False)
        flat[at] = val
    if rare_inf and flat.size > 8:
        flat[rng.choice(flat.size, 2, replace=False)] = (np.inf, -np.inf)
    if n > 2 and not rare_inf:
        S[1, :] = -np.inf
    if L > 3:
        S[:, 2] = np.nan
        S[:, 3] = 0.0
        S[::2, 3] = -0.0
    if n > 2:
        S[0] = np.nan
    return S


def _dev(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in xs)


def _np(*xs):
    return tuple(x.cpu().numpy() for x in xs)


# (n, L, Lr = m): one item; the smallest case with every special value; no multiple of any tile; a reference row 3 longer than
# the row kernel's LDS chunk; 5 columns more than the row kernel's tile; n and m one more than the column kernel's register tile
# and workgroup; long lines
SHAPES = [(1, 1, 1), (3, 4, 5), (130, 129, 257), (5, 70, ROW_CHUNK + 3), (3, ROW_TILE + 5, 9), (COL_TILE + 1, 70, COL_TILE + 1),
          (COL_BLOCK + 1, 70, COL_BLOCK + 1), (1000, 37, 1000)]


# ---- 1. the counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,M", SHAPES)
def test_counts_equal_the_restatements_integers(n, L, M):
    S, Rr, Q = _planted(n, L, 3 * n + L), _planted(n, M, 5 * n + M), _planted(M, L, 7 * M + L)
    St, Rt, Qt = _dev(S, Rr, Q)
    r2, c2 = ops.mp_row_counts(St, Rt), ops.mp_col_counts(St, Qt)
    row_cnt, col_cnt = ops.mp_line_counts(Rt, Qt)
    for t, shape in ((r2, (n, L)), (c2, (n, L)), (row_cnt, (n,)), (col_cnt, (L,))):
        assert t.dtype == torch.int32 and tuple(t.shape) == shape
    assert np.array_equal(r2.cpu().numpy(), MP.r2(S, Rr))
    assert np.array_equal(c2.cpu().numpy(), MP.r2(S.T, Q.T).T)
    assert np.array_equal(row_cnt.cpu().numpy(), MP.line_counts(Rr, 1)) and np.array_equal(col_cnt.cpu().numpy(), MP.line_counts(Q, 0))
    if n > 2 and L > 3:                                       # the cases this test is about are in the inputs
        assert np.isnan(S).any() and np.isinf(S).any() and (S == 0).any() and np.signbit(S[S == 0]).any()
        assert row_cnt[0] == 0 and col_cnt[2] == 0 and (r2.cpu().numpy()[np.isnan(S)] == 0).all()
    # a second run gives the same result
    assert torch.equal(ops.mp_row_counts(St, Rt), r2) and torch.equal(ops.mp_col_counts(St, Qt), c2)
    # either half of the line counts on its own
    assert torch.equal(ops.mp_line_counts(R=Rt)[0], row_cnt) and torch.equal(ops.mp_line_counts(Q=Qt)[1], col_cnt)
    assert ops.mp_line_counts(R=Rt)[1] is None and ops.mp_line_counts(Q=Qt)[0] is None


def test_counts_of_a_matrix_in_its_own_lines():
    n, L = 67, 70
    S = _planted(n, L, 19)
    St, = _dev(S)
    want = MP.counts(S)
    assert np.array_equal(ops.mp_row_counts(St, St).cpu().numpy(), want[0])
    assert np.array_equal(ops.mp_col_counts(St, St).cpu().numpy(), want[1])
    rc, cc = ops.mp_line_counts(St, St)
    assert np.array_equal(rc.cpu().numpy(), want[2]) and np.array_equal(cc.cpu().numpy(), want[3])


# ---- 2. accumulation over blocks of reference rows -------------------------------------------------------------------------------
def test_column_counts_accumulate_over_uneven_blocks():
    n, L, M = 70, 45, 130
    S, Q = _planted(n, L, 23), _planted(M, L, 24)
    St, Qt = _dev(S, Q)
    whole = ops.mp_col_counts(St, Qt)
    assert np.array_equal(whole.cpu().numpy(), MP.r2(S.T, Q.T).T)
    cuts = [0, 1, 1, 50, 67, 130]                             # a 1-row block, an empty one, uneven ones
    acc = torch.zeros((n, L), dtype=torch.int32, device=DEV)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out = ops.mp_col_counts(St, Qt[lo:hi], out=acc)
        assert out is acc
    assert torch.equal(acc, whole)
    # the first block overwrites (no buffer given), the others add
    acc = ops.mp_col_counts(St, Qt[:50])
    ops.mp_col_counts(St, Qt[50:], out=acc)
    assert torch.equal(acc, whole)
    # no reference row at all: zeros, and an accumulating call changes nothing
    assert int(ops.mp_col_counts(St, Qt[:0]).abs().sum()) == 0
    assert torch.equal(ops.mp_col_counts(St, Qt[:0], out=acc), whole)


def test_wrappers_refuse_bad_arguments_and_take_empty_slabs():
    St = torch.zeros((4, 8), device=DEV)
    i48 = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    i4, i8 = i48[:, 0].contiguous(), i48[0].contiguous()
    f4, f8 = torch.zeros((4,), device=DEV), torch.zeros((8,), device=DEV)
    with pytest.raises(ValueError):
        ops.mp_row_counts(St, St[:3])                         # another number of rows
    with pytest.raises(ValueError):
        ops.mp_col_counts(St, St[:, :7].contiguous())         # another number of columns
    with pytest.raises(ValueError):
        ops.mp_col_counts(St, St, out=i48[:3])
    with pytest.raises(ValueError):
        ops.mp_col_counts(St, St, out=St)                     # not int32
    with pytest.raises(ValueError):
        ops.mp_line_counts()
    with pytest.raises(ValueError):
        ops.mp_emp_apply(St, i48, i48, i8, i8)
    with pytest.raises(ValueError):
        ops.mp_emp_apply(St, i48, St, i4, i8)
    with pytest.raises(ValueError):
        ops.mp_gauss_apply(St, f4, f4, f8, f4)
    with pytest.raises(ValueError):
        ops.mp_moments_combine(torch.zeros((2, 3, 8), device=DEV))                   # not fp64
    with pytest.raises(ValueError):
        ops.mp_moments_combine(torch.zeros((2, 2, 8), dtype=torch.float64, device=DEV))
    assert ops.mp_row_counts(St[:0], St[:0]).shape == (0, 8) and ops.mp_col_counts(St[:0], St).shape == (0, 8)
    assert ops.mp_emp_apply(St[:0], i48[:0], i48[:0], i4[:0], i8).shape == (0, 8)
    assert ops.mp_gauss_apply(St[:0], f4[:0], f4[:0], f8, f8).shape == (0, 8)
    assert ops.mp_row_moments(St[:0])[0].shape == (0,)
    parts = ops.mp_col_moments(St[:0])                        # an empty slab: count 0 everywhere
    assert parts.shape == (3, 8) and parts.dtype == torch.float64 and float(parts.abs().sum()) == 0
    mean, sd = ops.mp_moments_combine(parts[None])
    assert torch.isnan(mean).all() and torch.isnan(sd).all()


# ---- 3. the emp apply ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,M", [(1, 1, 1), (3, 37, 5), (130, 129, 257), (90, 1000, 33)])
def test_emp_apply_is_bit_exact(n, L, M):
    S, Rr, Q = _planted(n, L, n + L), _planted(n, M, n + M), _planted(M, L, M + L)
    St, Rt, Qt = _dev(S, Rr, Q)
    r2, c2 = ops.mp_row_counts(St, Rt), ops.mp_col_counts(St, Qt)
    rc, cc = ops.mp_line_counts(Rt, Qt)
    T = ops.mp_emp_apply(St, r2, c2, rc, cc)
    got = T.cpu().numpy()
    want = MP.emp(S, Q, Rr)
    assert T.dtype == torch.float32 and _same_bits(got, want)
    assert np.isnan(got[np.isnan(S)]).all()                   # a NaN score stays NaN
    if n > 2:
        assert np.isnan(got[0]).all() and np.isnan(got[:, 2]).all() and np.isfinite(got).any()      # c = 0: the line is NaN
    assert _same_bits(ops.mp_emp_apply(St, r2, c2, rc, cc).cpu().numpy(), got)                       # a second run
    # a view misaligned by one float (the scalar path) gives the bits of the 16-byte path
    if L % 4 == 0 and n > 1:
        Sm = torch.empty(n * L + 1, device=DEV)[1:].view(n, L)
        Sm.copy_(St)
        assert Sm.data_ptr() % 16 == 4 and St.data_ptr() % 16 == 0
        assert _same_bits(ops.mp_emp_apply(Sm, r2, c2, rc, cc).cpu().numpy(), got)
        # so does every other operand the 16-byte path needs aligned, one at a time
        r2m = torch.empty(n * L + 1, dtype=torch.int32, device=DEV)[1:].view(n, L).copy_(r2)
        c2m = torch.empty(n * L + 1, dtype=torch.int32, device=DEV)[1:].view(n, L).copy_(c2)
        ccm = torch.empty(L + 1, dtype=torch.int32, device=DEV)[1:].copy_(cc)
        for args in ((r2m, c2, rc, cc), (r2, c2m, rc, cc), (r2, c2, rc, ccm)):
            assert sum(a.data_ptr() % 16 == 4 for a in args) == 1
            assert _same_bits(ops.mp_emp_apply(St, *args).cpu().numpy(), got)
    else:
        assert L % 4 != 0 or n == 1                           # L % 4 != 0: the scalar path was the one checked above


# ---- 4. moments and the gauss apply ----------------------------------------------------------------------------------------------
def _check_moments(got_mean, got_sd, want_mean, want_sd, infinities=True, atol=0):
    for got, want in ((got_mean, want_mean), (got_sd, want_sd)):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape
        if infinities:                                        # NaN and inf in the same places
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
            assert np.array_equal(got[np.isinf(got)], want[np.isinf(want)])
        fin = np.isfinite(want)
        assert np.isfinite(got[fin]).all()
        np.testing.assert_allclose(got[fin], want[fin], rtol=1e-6, atol=atol)


@pytest.mark.parametrize("n,L", [(1, 1), (3, 4), (130, 129), (257, 70), (37, 1000)])
def test_moments_are_the_fp64_restatements(n, L):
    X = _planted(n, L, 11 * n + L, rare_inf=True)
    Xt, = _dev(X)
    rm, rs = ops.mp_row_moments(Xt)
    want_r, want_c = MP.moments(X, 1), MP.moments(X, 0)
    _check_moments(rm, rs, *want_r)
    cm, cs = ops.mp_moments_combine(ops.mp_col_moments(Xt)[None])
    _check_moments(cm, cs, *want_c)
    if n > 2 and L > 3:
        assert np.isnan(want_r[0][0]) and np.isnan(want_c[0][2]) and want_c[1][3] == 0          # no entry; a column of zeros
        assert n * L < 1000 or (np.isfinite(want_r[1]).sum() > n // 2 and np.isfinite(want_c[1]).sum() > L // 2)
    # a second run gives the same bits; the rows fed as slabs cut at uneven places (an empty one among them) give the same
    # moments to 1e-6.  The triples carry means, and c fl(sum / c) is the sum only to 2^-53 of it: where a line's mean cancels to
    # exactly 0 (this grid does that) the recombined mean is about 1e-17 of the line's scale instead, hence the absolute term.
    assert _same_bits(ops.mp_row_moments(Xt)[0].cpu().numpy(), rm.cpu().numpy())
    cuts = sorted({0, min(1, n), min(1, n), n // 3, n})
    parts = torch.stack([ops.mp_col_moments(Xt[lo:hi]) for lo, hi in zip([0] + cuts, cuts + [n])])
    cm2, cs2 = ops.mp_moments_combine(parts)
    _check_moments(cm2, cs2, *want_c, atol=1e-12)
    again = ops.mp_moments_combine(parts)
    assert _same_bits(again[0].cpu().numpy(), cm2.cpu().numpy()) and _same_bits(again[1].cpu().numpy(), cs2.cpu().numpy())


def _stated_matrix(seed=11, n=96, hub=5):
    """test_localscale_gpu._stated_matrix: scores on a grid of 1/256: noise, +0.25 for the true pairs, +0.3125 on one video's
    whole column (the hub)."""
    rng = np.random.default_rng(seed)
    S = np.round(rng.standard_normal((n, n)) * 32) / 256
    S[np.arange(n), np.arange(n)] += 0.25
    S[:, hub] += 0.3125
    return np.clip(S, -1, 1).astype(np.float32)


def _gauss_bar(S, moments):
    """4 x the relative distance of the float32 restatement from the fp64 formulas on these inputs (the factor DESIGN.md 6.4 uses,
    for the same reason: the device erfcf and a third order of operations)."""
    want = MP.gauss_scores(S, *moments, dtype=np.float64)
    return want, 4 * MP.rel_distance(MP.gauss_scores(S, *moments), want)


def _gauss_reference(S, Qt=None, Qv=None):
    """(want, bar) for T of one rank: the fp64 formulas on the GPU's own one-slab moments of the lines, and _gauss_bar."""
    rows, cols = _dev(S if Qv is None else Qv, S if Qt is None else Qt)
    moments = _np(*ops.mp_row_moments(rows), *ops.mp_moments_combine(ops.mp_col_moments(cols)[None]))
    return _gauss_bar(S, moments)


MEASURABLE = 1000            # finite entries below which a measured bar says nothing (it can be 0): placement and paths are checked


@pytest.mark.parametrize("which", ["hub96", "hub1000", "planted130x129"])
def test_gauss_apply_is_within_four_times_the_restatements_own_distance(which):
    S = {"hub96": lambda: _stated_matrix(), "hub1000": lambda: _stated_matrix(n=1000),
         "planted130x129": lambda: _planted(130, 129, 5, rare_inf=True)}[which]()
    St, = _dev(S)
    n, L = S.shape
    rm, rs = ops.mp_row_moments(St)                            # the GPU's own moments
    cm, cs = ops.mp_moments_combine(ops.mp_col_moments(St)[None])
    moments = _np(rm, rs, cm, cs)
    T = ops.mp_gauss_apply(St, rm, rs, cm, cs)
    got = T.cpu().numpy()
    want, bar = _gauss_bar(S, moments)
    dist = MP.rel_distance(got, want)
    print(f"gauss apply {which}: GPU distance from the fp64 formulas {dist:.3e}, bar {bar:.3e}")
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert (got[want == 0] == 0).all()
    assert np.isfinite(want).sum() > want.size // 2 and bar > 0
    assert dist <= bar
    assert _same_bits(ops.mp_gauss_apply(St, rm, rs, cm, cs).cpu().numpy(), got)                    # a second run


@pytest.mark.parametrize("n,L", [(1, 1), (3, 4), (5, 37), (130, 128)])
def test_gauss_apply_paths_agree_and_nan_stays_nan(n, L):
    S = _planted(n, L, 13 * n + L, rare_inf=True)
    St, = _dev(S)
    rm, rs = ops.mp_row_moments(St)
    cm, cs = ops.mp_moments_combine(ops.mp_col_moments(St)[None])
    got = ops.mp_gauss_apply(St, rm, rs, cm, cs).cpu().numpy()
    want = MP.gauss_scores(S, *_np(rm, rs, cm, cs), dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[np.isnan(S)]).all()
    fin = np.isfinite(want)
    assert (got[fin] <= 0).all() and (got[fin] >= -1).all()   # MP - 1 of a probability
    if L % 4 == 0 and n > 1:                                  # the scalar path gives the bits of the 16-byte path
        Sm = torch.empty(n * L + 1, device=DEV)[1:].view(n, L)
        Sm.copy_(St)
        assert Sm.data_ptr() % 16 == 4 and St.data_ptr() % 16 == 0
        assert _same_bits(ops.mp_gauss_apply(Sm, rm, rs, cm, cs).cpu().numpy(), got)
        # so does a column vector misaligned by one float, one at a time
        cmm, csm = (torch.empty(L + 1, device=DEV)[1:].copy_(x) for x in (cm, cs))
        assert cmm.data_ptr() % 16 == 4 and csm.data_ptr() % 16 == 4 and cm.data_ptr() % 16 == 0 and cs.data_ptr() % 16 == 0
        assert _same_bits(ops.mp_gauss_apply(St, rm, rs, cmm, cs).cpu().numpy(), got)
        assert _same_bits(ops.mp_gauss_apply(St, rm, rs, cm, csm).cpu().numpy(), got)


# ---- 5. the same bits whatever the split -----------------------------------------------------------------------------------------
def _emulated(W, fn):
    world = comm.EmulatedWorld(W, real_collectives=False)
    out = {}

    def run(r):
        c = world.comm(r)
        with comm.use(c):
            c.begin_step()
            out[r] = fn(SimpleNamespace(world_size=W), r)
    world.settle(run)
    return [out[r] for r in range(W)]


# (n, L, bank texts, bank videos, rows per gathered block): 5 bank texts leave three of 8 ranks without one; 5 test texts leave
# three of 8 ranks with an empty slab; 16 rows per block: several collectives, the last block short and uneven over the ranks
@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("n,L,M_t,M_v,B", [(101, 67, 5, 11, 256), (101, 67, 45, 11, 16), (5, 9, 3, 4, 256)])
def test_the_matrix_has_the_same_bits_for_every_world_size(n, L, M_t, M_v, B, bank, monkeypatch):
    monkeypatch.setattr(evaluator, "MP_GATHER_ROWS", B)
    S, Qt, Qv = _planted(n, L, 31, rare_inf=True), _planted(M_t, L, 32, rare_inf=True), _planted(n, M_v, 33, rare_inf=True)
    St, Qt_t, Qv_t = _dev(S, Qt, Qv)
    lines = (Qt, Qv) if bank else (None, None)
    want_emp = MP.emp(S, *lines)
    want64, bar = _gauss_reference(S, *lines)
    first = {}
    for W in (1, 2, 3, 8):
        def fn(a, r, W=W):
            r0, r1 = evaluator.slab_bounds(n, W, r)
            q0, q1 = evaluator.slab_bounds(M_t, W, r)
            slabs = (Qt_t[q0:q1].contiguous(), Qv_t[r0:r1].contiguous()) if bank else None
            src = slabs[0] if bank else St[r0:r1].contiguous()
            out = {mode: evaluator._mutual_proximity_from_slab(St[r0:r1].contiguous(), n, L, W, r, mode, slabs, M_t if bank else None)
                   .cpu().numpy() for mode in MODES}
            out["moments"] = _np(*evaluator._mp_column_moments(src, W))
            return out
        outs = _emulated(W, fn)
        T = {mode: np.concatenate([o[mode] for o in outs]) for mode in MODES}
        assert T["emp"].shape == (n, L)
        # emp: the restatement's bits, for every W
        assert _same_bits(T["emp"], want_emp), W
        # gauss: the column moments are the same bits on every rank; T stays within the bar across W
        for o in outs:
            assert _same_bits(o["moments"][0], outs[0]["moments"][0]) and _same_bits(o["moments"][1], outs[0]["moments"][1]), W
        assert np.array_equal(np.isnan(T["gauss"]), np.isnan(want64)), W
        if W == 1:
            first = T
            if np.isfinite(want64).sum() >= MEASURABLE:
                assert MP.rel_distance(T["gauss"], want64) <= bar
        else:                                                 # the column moments combine in another order: last bits
            assert MP.rel_distance(T["gauss"], first["gauss"].astype(np.float64)) <= bar, W


# ---- 6. the sharded evaluator ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model():
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _testset(n=N, seed=4242):
    t, v, tm, vm = synth.make_samples(seed, "test", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, v, tm.astype(np.float32), vm.astype(np.float32)))


@functools.lru_cache(maxsize=None)
def _bank(n=40, seed=77):
    t, v, tm, vm = synth.make_samples(seed, "train", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, tm.astype(np.float32), v, vm.astype(np.float32)))


def _full(m, a, b, am, bm, W):
    n = a.shape[0]
    return np.concatenate([evaluator._slab_similarity(m, a, b, am, bm, *evaluator.slab_bounds(n, W, r)).cpu().numpy()
                           for r in range(W)])


@functools.lru_cache(maxsize=None)
def _split_scores(W):
    """(S, Qt, Qv) of the test set and the bank as W slabs score them: computed once per W, shared, not written to."""
    m, (t, v, tm, vm), bank = _model(), _testset(), _bank()
    out = _full(m, t, v, tm, vm, W), _full(m, bank[0], v, bank[1], vm, W), _full(m, t, bank[2], tm, bank[3], W)
    for a in out:
        a.setflags(write=False)
    return out


def _same_metrics(a, b):
    assert set(a) == set(b)
    for key in a:
        if key == "hubness":
            for hk in a[key]:
                if isinstance(a[key][hk], np.ndarray):
                    assert np.array_equal(a[key][hk], b[key][hk]), hk
                else:
                    assert a[key][hk] == b[key][hk], hk
        else:
            assert a[key] == b[key], key


@functools.lru_cache(maxsize=None)
def _one_rank(mode, bank):
    """T of the test set from one rank: computed once, shared, not written to."""
    T = evaluator.sharded_mutual_proximity_slab(_model(), *_testset(), SimpleNamespace(world_size=1), mode, bank=bank,
                                                querybank=_bank() if bank else None).cpu().numpy()
    T.setflags(write=False)
    return T


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_evaluator_under_emulated_ranks_equals_the_restatement(mode, W, bank):
    m = _model()
    t, v, tm, vm = _testset()
    qb = _bank() if bank else None

    def fn(a, r):
        T = evaluator.sharded_mutual_proximity_slab(m, t, v, tm, vm, a, mode, bank=bank, querybank=qb)
        met = evaluator.sharded_mutual_proximity_metrics(m, t, v, tm, vm, a, mode, bank=bank, querybank=qb, hubness_k=5)
        return T.cpu().numpy(), met
    outs = _emulated(W, fn)
    T = np.concatenate([o[0] for o in outs])
    for _, met in outs:                                       # every rank returns the same dictionaries
        _same_metrics(met[0], outs[0][1][0])
        _same_metrics(met[1], outs[0][1][1])
    t2v, v2t = outs[0][1]
    for d in (t2v, v2t):
        assert d["mode"] == mode and d["bank"] is bank and "k" not in d and "beta" not in d
    # T against the definition, from the same split's S (and Qt, Qv)
    S, Qt, Qv = _split_scores(W)
    lines = (Qt, Qv) if bank else (None, None)
    one = _split_scores(1)
    same_inputs = _same_bits(S, one[0]) and (not bank or (_same_bits(Qt, one[1]) and _same_bits(Qv, one[2])))
    if mode == "emp":
        ref = MP.emp(S, *lines)
        assert _same_bits(T, ref)                             # the restatement's bits
        if same_inputs:                                       # and so the same bits for every W
            assert _same_bits(T, _one_rank(mode, bank))
    else:
        want64, bar = _gauss_reference(S, *lines)
        assert np.isfinite(want64).all() and bar > 0
        dist = MP.rel_distance(T, want64 if W == 1 or not same_inputs else _one_rank(mode, bank))
        print(f"gauss evaluator W = {W}, bank = {bank}: distance {dist:.3e} from {'the fp64 formulas' if W == 1 else 'one rank'}, "
              f"bar {bar:.3e}")
        assert dist <= bar
        ref = T                                               # the metrics of the GPU's own T: a last bit cannot flip a rank
    assert t2v["cols"] == R.single_ranks(ref).tolist() and v2t["cols"] == R.single_ranks(ref.T).tolist()
    ht, hv = H.hubness(ref, 5)
    assert np.array_equal(t2v["hubness"]["occurrence"], ht["occ"]) and np.array_equal(v2t["hubness"]["occurrence"], hv["occ"])


def test_metrics_with_mutual_proximity_keep_the_raw_dictionaries():
    m = _model()
    t, v, tm, vm = _testset()
    a = SimpleNamespace(world_size=1)
    raw = evaluator.sharded_metrics_with_hubness(m, t, v, tm, vm, a, 5)
    plain = evaluator.sharded_metrics(m, t, v, tm, vm, a)
    for mode in MODES:
        both = evaluator.sharded_metrics_with_mutual_proximity(m, t, v, tm, vm, a, mode, hubness_k=5)
        alone = evaluator.sharded_mutual_proximity_metrics(m, t, v, tm, vm, a, mode, hubness_k=5)
        for d in range(2):
            _same_metrics({k_: v_ for k_, v_ in both[d].items() if k_ != "mutual_proximity"}, raw[d])
            _same_metrics(both[d]["mutual_proximity"], alone[d])
        nohub = evaluator.sharded_metrics_with_mutual_proximity(m, t, v, tm, vm, a, mode)
        for d in range(2):
            _same_metrics({k_: v_ for k_, v_ in nohub[d].items() if k_ != "mutual_proximity"}, plain[d])
            assert "hubness" not in nohub[d]["mutual_proximity"]
    with pytest.raises(ValueError):
        evaluator.sharded_mutual_proximity_metrics(m, t, v, tm, vm, a, "csls")
    with pytest.raises(ValueError):
        evaluator.sharded_mutual_proximity_metrics(m, t, v, tm, vm, a, "emp", hubness_k=129)


# ---- 7. several sentences per video -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_multi_sentence_fixture_under_emulated_ranks(mode):
    g = golden("multi_sentence")
    S, cut = g["S"].astype(np.float32), g["cut_off_points"].tolist()
    Ns, V_ = S.shape
    ends = np.asarray(cut, dtype=np.int64) + 1
    St = torch.from_numpy(S).to(DEV)
    want32 = MP.mutual_proximity(S, mode)
    want64, bar = _gauss_reference(S)
    first = None
    for W in (1, 2, 3):
        def fn(a, r, W=W):
            r0, r1 = evaluator.slab_bounds(Ns, W, r)
            T = evaluator._mutual_proximity_from_slab(St[r0:r1].contiguous(), Ns, V_, W, r, mode)
            return T.cpu().numpy(), evaluator._metrics_from_normalised(T, T, Ns, V_, W, r, ends, 3)
        outs = _emulated(W, fn)
        T = np.concatenate([o[0] for o in outs])
        for o in outs:
            _same_metrics(o[1][0], outs[0][1][0])
            _same_metrics(o[1][1], outs[0][1][1])
        t2v, v2t = outs[0][1]
        # a video's line is every sentence's score for it: the restatement's columns over the sentence rows
        if mode == "emp":
            assert _same_bits(T, want32)
            ref = want32
        else:
            first = T if W == 1 else first
            assert np.array_equal(np.isnan(T), np.isnan(want64)) and MP.rel_distance(T, want64 if W == 1 else first) <= bar
            ref = T
        want_t = training.RetrievalMetrics.multi_sentence_metrics_from_ranks(R.group_ranks(ref, cut))
        want_v = training.RetrievalMetrics.metrics_from_ranks(R.single_ranks(R.group_max(ref, cut)))
        for key in ("R1", "R5", "R10", "MedianR", "MeanR"):
            assert t2v[key] == want_t[key] and v2t[key] == want_v[key], (W, key)
        ht, hv = H.hubness(ref, 3, cut)
        assert np.array_equal(t2v["hubness"]["occurrence"], ht["occ"]) and np.array_equal(v2t["hubness"]["occurrence"], hv["occ"])


# ---- 8. two gloo ranks, one child process each ----------------------------------------------------------------------------------
GLOO_CASES = (("emp", False), ("gauss", True), ("emp", True))


def _gloo_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    args = SimpleNamespace(world_size=world, local_rank=rank)
    m = _model()
    t, v, tm, vm = _testset()
    res = {(mode, bank): evaluator.sharded_mutual_proximity_metrics(m, t, v, tm, vm, args, mode, bank=bank, querybank=_bank(), hubness_k=5)
           for mode, bank in GLOO_CASES}
    torch.save(res, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_the_emulated_ranks_and_a_single_process(tmp_path):
    m = _model()
    t, v, tm, vm = _testset()
    world, port = 2, 29697
    out = str(tmp_path / "res")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--gloo-worker", str(r), str(world), str(port), out],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs, failed = [], False
    for p in procs:                                          # every child under its own time limit
        try:
            logs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            failed = True
            for q in procs:
                q.kill()
            logs.append(p.communicate()[0])
    assert not failed and all(p.returncode == 0 for p in procs), "\n".join(log[-2000:] for log in logs)
    for mode, bank in GLOO_CASES:
        def fn(a, r, mode=mode, bank=bank):
            return evaluator.sharded_mutual_proximity_metrics(m, t, v, tm, vm, a, mode, bank=bank, querybank=_bank(), hubness_k=5)
        want = _emulated(world, fn)[0]
        one = fn(SimpleNamespace(world_size=1), 0)
        for r in range(world):
            res = torch.load(f"{out}.{r}", weights_only=False)[(mode, bank)]
            for d in range(2):
                _same_metrics(res[d], want[d])
                if mode == "emp":                             # the same bits for every world size: the same metrics
                    _same_metrics(res[d], one[d])


# ---- 9. the feature does what it claims -------------------------------------------------------------------------------------------
def _hub_bank(hub=5, n=96, M=64, seed=12):
    """A 64-item bank on the grid of _stated_matrix: the bank's texts see the same hub column (Qt [M, n]), the test texts see the
    bank's videos as noise (Qv [n, M])."""
    rng = np.random.default_rng(seed)
    Qt = np.round(rng.standard_normal((M, n)) * 32) / 256
    Qt[:, hub] += 0.3125
    Qv = np.round(rng.standard_normal((n, M)) * 32) / 256
    return np.clip(Qt, -1, 1).astype(np.float32), Qv.astype(np.float32)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_mutual_proximity_takes_a_planted_hub_out_of_the_lists(mode, bank):
    hub, k, n = 5, 5, 96
    S = _stated_matrix()
    raw_occ = H.hubness(S, k)[0]["occ"]
    assert raw_occ[hub] == raw_occ.max() == 74               # the hub sits in 74 of the 96 top-5 lists
    lines = _hub_bank() if bank else (None, None)
    Tr = MP.mutual_proximity(S, mode, *lines)
    ref = H.hubness(Tr, k)
    # the restatement alone: emp 74 -> 10 and R@1 20.0 -> 30.4, gauss 74 -> 14 and 20.0 -> 33.3; this bank: 74 -> 10 (emp), 13 (gauss)
    assert 2 * ref[0]["occ"][hub] <= raw_occ[hub], (mode, ref[0]["occ"][hub])
    if not bank:                                              # recall under the project's own tie rule does not fall
        assert R.recall(R.single_ranks(Tr), 1) >= R.recall(R.single_ranks(S), 1)
    # the GPU's lists and ranks are the restatement's (gauss: those of its own T, which is the restatement's to the bar)
    slabs = tuple(_dev(*lines)) if bank else None
    T = evaluator._mutual_proximity_from_slab(torch.from_numpy(S).to(DEV), n, n, 1, 0, mode, slabs, 64 if bank else None)
    t2v, v2t = evaluator._metrics_from_normalised(T, T, n, n, 1, 0, None, k)
    if mode == "emp":
        assert _same_bits(T.cpu().numpy(), Tr)
    else:
        want64, bar = _gauss_reference(S, *lines)
        assert MP.rel_distance(T.cpu().numpy(), want64) <= bar
        Tr = T.cpu().numpy()
        ref = H.hubness(Tr, k)
        assert 2 * ref[0]["occ"][hub] <= raw_occ[hub], (mode, ref[0]["occ"][hub])
    assert np.array_equal(t2v["hubness"]["occurrence"], ref[0]["occ"]) and np.array_equal(v2t["hubness"]["occurrence"], ref[1]["occ"])
    assert t2v["cols"] == R.single_ranks(Tr).tolist() and v2t["cols"] == R.single_ranks(Tr.T).tolist()
    assert t2v["R1"] == R.recall(R.single_ranks(Tr), 1)
    if not bank:
        assert t2v["R1"] >= R.recall(R.single_ranks(S), 1)


# ---- 10. eval_epoch and main_retrieval.py ---------------------------------------------------------------------------------------------
class Loader:
    def __init__(self, batches, dataset=None):
        self.batches, self.dataset = batches, dataset

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _batches(t, v, tm, vm, order, bs):
    return [(t[ix], tm[ix].long(), v[ix], vm[ix].long(), ix.clone(), ix.clone())
            for ix in (order[lo:lo + bs] for lo in range(0, len(order), bs))]


def _args(**over):
    return SimpleNamespace(world_size=1, rank=0, local_rank=0, logger=logging.getLogger("test_mutualprox"), **over)


def _fresh_model(bank=None):
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    m = m.to(DEV).eval()
    if bank is not None:
        m.mb_ind = torch.arange(bank[0].shape[0], device=DEV)
        m.mb_feat_t, m.mb_mask_t, m.mb_feat_v, m.mb_mask_v = bank
    return m


def test_eval_epoch_single_sentence_with_each_mode(caplog):
    t, v, tm, vm = (x.cpu() for x in _testset())
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    loader = Loader(_batches(t, v, tm, vm, order, 32))
    bank = _bank()
    dev = torch.device(DEV)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="test_mutualprox"):
        base = training.eval_epoch(_args(), _fresh_model(), loader, dev)
    assert not any("MP-" in r.getMessage() for r in caplog.records)                  # without the flag: no tagged line
    assert "mutual_proximity" not in base[0] and "mutual_proximity" not in base[1]
    assert training.eval_epoch(_args(mutual_proximity="none"), _fresh_model(), loader, dev) == base
    want_raw = evaluator.sharded_metrics(_model(), *_testset(), _args())
    assert base[0] == want_raw[0] and base[1] == want_raw[1]  # without the flag: what the evaluator gave before
    for mode, with_bank in (("emp", False), ("gauss", True), ("emp", True), ("gauss", False)):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="test_mutualprox"):
            on = training.eval_epoch(_args(mutual_proximity=mode, mutual_proximity_bank=int(with_bank), hubness_k=5),
                                     _fresh_model(bank), loader, dev)
        lines = [r.getMessage() for r in caplog.records]
        tag = evaluator.mutual_proximity_label(mode, with_bank)
        assert tag == f"[{'QB-' if with_bank else ''}MP-{mode}]"
        assert any(line.startswith(f"Text-to-Video {tag}: R@1") for line in lines), lines
        assert any(line.startswith(f"Video-to-Text {tag}: R@1") for line in lines)
        assert sum(f"{tag} Hubness@5" in line for line in lines) == 2
        strip = [{k_: v_ for k_, v_ in d.items() if k_ not in ("mutual_proximity", "hubness")} for d in on]
        assert strip[0] == base[0] and strip[1] == base[1]
        want = evaluator.sharded_mutual_proximity_metrics(_model(), *_testset(), _args(), mode, bank=with_bank, querybank=bank,
                                                          hubness_k=5)
        _same_metrics(on[0]["mutual_proximity"], want[0])
        _same_metrics(on[1]["mutual_proximity"], want[1])
    with pytest.raises(ValueError, match="load_memory_bank"):
        training.eval_epoch(_args(mutual_proximity="emp", mutual_proximity_bank=1), _fresh_model(), loader, dev)
    for other in (dict(test_norm="is"), dict(local_scaling="csls")):
        with pytest.raises(ValueError, match="mutual_proximity"):
            training.eval_epoch(_args(mutual_proximity="emp", **other), _fresh_model(), loader, dev)


def test_eval_epoch_multi_sentence_with_emp():
    Vn = 41
    sizes = 1 + (np.arange(Vn) * 3) % 4
    ends = np.cumsum(sizes)
    Ns = int(ends[-1])
    grp = np.searchsorted(ends, np.arange(Ns), side="right")
    t, _, tm, _ = (torch.from_numpy(a) for a in synth.make_samples(92, "test", Ns, Nt, Nv))
    _, v, _, vm = (torch.from_numpy(a) for a in synth.make_samples(93, "test", Vn, Nt, Nv))
    t = t + 0.4 * v[grp].mean(1, keepdim=True)
    dataset = SimpleNamespace(multi_sentence_per_video=True, cut_off_points=ends.tolist(), sentence_num=Ns, video_num=Vn)
    loader = Loader(_batches(t, v[grp], tm, vm[grp], torch.arange(Ns), 16), dataset)
    dev = torch.device(DEV)
    base = training.eval_epoch(_args(), _fresh_model(), loader, dev)
    on = training.eval_epoch(_args(mutual_proximity="emp"), _fresh_model(), loader, dev)
    for d in range(2):
        assert {k_: v_ for k_, v_ in on[d].items() if k_ != "mutual_proximity"} == base[d]
    want = evaluator.sharded_mutual_proximity_metrics(_model(), t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float(), _args(),
                                                      "emp", cut_off_points=(ends - 1).tolist())
    _same_metrics(on[0]["mutual_proximity"], want[0])
    _same_metrics(on[1]["mutual_proximity"], want[1])


def test_main_retrieval_logs_mutual_proximity_only_with_the_flag():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--synthetic_test", "200"]
    outs = []
    for extra in ([], ["--mutual_proximity", "emp"],
                  ["--mutual_proximity", "gauss", "--mutual_proximity_bank", "1", "--hubness_k", "5"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()])
    plain, emp, qb = outs
    assert not any("MP-" in line or "mutual_proximity" in line for line in plain)
    extra_emp = [line for line in emp if "[MP-emp]" in line]
    assert len(extra_emp) == 1 and extra_emp[0].startswith("text->video [MP-emp] R@1")
    assert "video->text [MP-emp] R@1" in extra_emp[0]
    assert [line for line in emp if "[MP-" not in line] == plain          # the raw lines: those of a run without the flag
    extra_qb = [line for line in qb if "[QB-MP-gauss]" in line]
    assert len(extra_qb) == 3 and sum("Hubness@5" in line for line in extra_qb) == 2
    raw_qb = [line for line in qb if "[QB-MP-" not in line and "Hubness@" not in line and "memory bank" not in line]
    assert raw_qb == plain


if __name__ == "__main__":                                   # one gloo rank of the two-rank test
    if len(sys.argv) == 6 and sys.argv[1] == "--gloo-worker":
        _gloo_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
