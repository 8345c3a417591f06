"""GPU: test-time Sinkhorn normalisation (neighborretr_amd/csrc/nr_sinknorm.hip, evaluator modes "sinkhorn" / "qbsinkhorn").

The yardstick is the fp64 restatement (sinknorm_ref), never the GPU.  The bar of every comparison of values is MEASURED ON THE
CPU on the very inputs of the test: the distance of the float32 restatement (the definition's roundings, NumPy's summation
order) from the fp64 one, times 4 -- the GPU sums in another order than NumPy, and two NumPy orders (columns permuted) already
differ by 2x, so 4x is that spread doubled.  Measured here (max |dT|, float32 against fp64): 0.9e-5 at (1000, 1000) after 50
iterations, values up to 26; bar 3.8e-5.  u and v get bars of their own, measured the same way (a common shift of u against
v leaves T alone and is not damped by the iteration, so their distances are not T's).  Every figure is printed before it is
asserted.

Metrics (ranks, R@K, hubness occurrences) are compared exactly, on seeded sets the fp64 restatement alone finds well separated
(no rank-deciding pair and no list boundary within a relative 1e-4)."""
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
import sinknorm_ref as K
from neighborretr_amd import comm, evaluator, modeling, ops, synth, training
from util import golden, params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BETA = 20.0
N, Nt, Nv = 96, 24, 12
MODES = ("sinkhorn", "qbsinkhorn")
SPREAD = 4.0                                                # GPU bar = SPREAD x (float32 restatement - fp64 restatement)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _dist(a, b):
    """max |a - b| over the entries where both are finite; the non-finite entries must agree exactly."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)])
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0


def _within(what, gpu, f32, f64):
    """The GPU's distance from the fp64 restatement against SPREAD x the float32 restatement's, both printed."""
    d_gpu, d_32 = _dist(gpu, f64), _dist(f32, f64)
    print(f"{what}: GPU - fp64 {d_gpu:.3e}   float32 - fp64 {d_32:.3e}   bar {SPREAD * d_32:.3e}")
    assert d_gpu <= SPREAD * d_32, (what, d_gpu, d_32)
    return d_gpu, d_32


def _planted(n, L, seed):
    """The awkward slab of test_hubnorm_gpu.py (signed zeros, -inf, NaN, whole lines of them) with ONE +inf entry: a +inf takes
    its row and its column out of the balancing, so more of them would leave nothing to check."""
    rng = np.random.default_rng(seed)
    S = (np.round(rng.standard_normal((n, L)) * 8) / 32).astype(np.float32)
    flat = S.reshape(-1)
    for val, frac in ((0.0, 0.05), (-0.0, 0.05), (-np.inf, 0.02), (np.nan, 0.05)):
        at = rng.choice(flat.size, max(1, int(frac * flat.size)), replace=False)
        flat[at] = val
    if n > 2:
        S[0] = np.nan                                         # a row that is entirely NaN
        S[1, :] = -np.inf                                     # a row of -inf only
        S[n - 1, L - 1] = np.inf
    if L > 3:
        S[:, 2] = np.nan                                      # a column that is entirely NaN
        S[:, 3] = 0.0
        S[::2, 3] = -0.0                                      # a column of signed zeros only
    return S


def _hub_matrix(n, L, seed, hub=3, own=None):
    rng = np.random.default_rng(seed)
    S = (rng.standard_normal((n, L)) * 0.1).astype(np.float32)
    own = np.arange(n) % L if own is None else own
    S[np.arange(n), own] += 0.35
    S[:, hub] += 0.25
    return S


def _misaligned(t):
    """A copy of t whose storage starts 4 bytes off a 16-byte boundary: the scalar load paths."""
    out = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# ---- 1. the half-steps and the apply against the definition ---------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 37), (130, 129), (90, 1000), (3, 20000)]


def _half_ref(S, u, v, log_mu, log_nu, dtype):
    """(u', v', T) of the definition from given potentials: the row half-step from v, the column half-step from u, T from
    (u, v), every input a float32 carried in `dtype`."""
    A = K.beta_s(S, BETA, dtype)
    c = lambda x: np.asarray(x, dtype=np.float32).astype(dtype)                 # noqa: E731
    return K._half(A, c(v), c(log_mu), 1), K._half(A, c(u), c(log_nu), 0), K.plan(S, BETA, c(u), c(v), dtype)


@pytest.mark.parametrize("n,L", SHAPES)
def test_half_steps_and_apply_equal_the_definition(n, L):
    S = _planted(n, L, 7 * n + L)
    rng = np.random.default_rng(n + L)
    u = (rng.standard_normal(n) * 2).astype(np.float32)
    v = (rng.standard_normal(L) * 2).astype(np.float32)
    log_mu = (-np.log(n) + 0.1 * rng.standard_normal(n)).astype(np.float32)
    log_nu = (-np.log(L) + 0.1 * rng.standard_normal(L)).astype(np.float32)
    want64, want32 = (_half_ref(S, u, v, log_mu, log_nu, dt) for dt in (np.float64, np.float32))
    St, ut, vt, mut, nut = (_dev(a) for a in (S, u, v, log_mu, log_nu))
    variants = [("aligned", St, vt)]
    if L % 4 == 0 and n > 1:
        variants += [("scalar S", _misaligned(St), vt), ("scalar v", St, _misaligned(vt))]
    for name, Sx, vx in variants:
        got_u = ops.sinknorm_row(Sx, BETA, vx, mut)
        stats = ops.sinknorm_col_stats(Sx, BETA, ut)
        got_v = ops.sinknorm_finish_cols(stats[None].contiguous(), nut)
        direct = ops.sinknorm_finish_cols(ops.sinknorm_col_stats(Sx, BETA, ut, want_stats=False), nut)
        got_T = ops.sinknorm_apply(Sx, BETA, ut, vx)
        # a second run gives the same bits; finishing from the blocks' pairs = finishing from their merge
        assert _same_bits(ops.sinknorm_row(Sx, BETA, vx, mut).cpu().numpy(), got_u.cpu().numpy())
        assert _same_bits(ops.sinknorm_col_stats(Sx, BETA, ut).cpu().numpy(), stats.cpu().numpy())
        assert _same_bits(direct.cpu().numpy(), got_v.cpu().numpy())
        got_u, got_v, got_T = got_u.cpu().numpy(), got_v.cpu().numpy(), got_T.cpu().numpy()
        # lines without a finite LSE keep potential 0, exactly
        assert np.array_equal(got_u == 0, want64[0] == 0) and np.array_equal(got_v == 0, want64[1] == 0)
        _within(f"({n},{L}) {name} row half-step u", got_u, want32[0], want64[0])
        _within(f"({n},{L}) {name} column half-step v", got_v, want32[1], want64[1])
        # the apply is three roundings per entry: the float32 restatement's bits (NaN stays NaN)
        nan = np.isnan(want32[2])
        assert np.array_equal(np.isnan(got_T), nan) and np.array_equal(nan, np.isnan(S))
        assert _same_bits(got_T[~nan], want32[2][~nan])
    if variants[1:]:                                          # a column's pairs do not depend on the load width
        assert _same_bits(ops.sinknorm_col_stats(St, BETA, ut).cpu().numpy(),
                          ops.sinknorm_col_stats(_misaligned(St), BETA, ut).cpu().numpy())


def test_half_steps_of_an_empty_slab():
    S = torch.empty((0, 17), device=DEV)
    none = torch.empty((0,), device=DEV)
    nu = torch.full((17,), -1.5, device=DEV)
    assert ops.sinknorm_row(S, BETA, torch.zeros(17, device=DEV), none).numel() == 0
    stats = ops.sinknorm_col_stats(S, BETA, none)
    assert torch.all(stats[0] == float("-inf")) and torch.all(stats[1] == 0)
    assert torch.all(ops.sinknorm_finish_cols(stats[None].contiguous(), nu) == 0)         # no entry: potential 0
    assert torch.all(ops.sinknorm_finish_cols(ops.sinknorm_col_stats(S, BETA, none, want_stats=False), nu) == 0)
    assert ops.sinknorm_apply(S, BETA, none, torch.zeros(17, device=DEV)).shape == (0, 17)
    u, v, err = evaluator._sinkhorn_potentials(S, BETA, none, nu, 3, 1)
    assert u.numel() == 0 and torch.all(v == 0) and err == 0.0


# ---- 2. n_iter iterations against the fp64 restatement -------------------------------------------------------------------------------
def _sizes(L, n):
    g = 1 + (np.arange(L) * 3) % 5
    assert g.sum() == n
    return g


CASES = [(96, 96, None), (600, 200, "groups"), (1000, 1000, None)]


@pytest.mark.parametrize("n,L,marg", CASES)
def test_potentials_and_plan_against_the_fp64_restatement(n, L, marg):
    """Bars measured on the CPU, on these inputs (float32 restatement - fp64 restatement, x 4).  Seen: (1000, 1000), 50
    iterations: max |dT| 0.9e-5 (bar 3.8e-5), |du|, |dv| about 1e-5."""
    cut = None if marg is None else (np.cumsum(_sizes(L, n)) - 1).tolist()
    own = None if cut is None else np.searchsorted(np.asarray(cut) + 1, np.arange(n), side="right")
    S = _hub_matrix(n, L, 100 + n, own=own)
    St = _dev(S)
    ends = None if cut is None else np.asarray(cut) + 1
    log_mu, log_nu = evaluator._log_marginals(n, L, ends, DEV)
    want_mu, want_nu = K.marginals(n, L, cut, np.float32)
    assert _same_bits(log_mu.cpu().numpy(), want_mu) and _same_bits(log_nu.cpu().numpy(), want_nu)
    errs = {}
    for n_iter in (1, 5, 50):
        T64, u64, v64, e64 = K.sinkhorn(S, BETA, n_iter, cut)
        T32, u32, v32, e32 = K.sinkhorn(S, BETA, n_iter, cut, dtype=np.float32)
        u, v, err = evaluator._sinkhorn_potentials(St, BETA, log_mu, log_nu, n_iter, 1)
        T = ops.sinknorm_apply(St, BETA, u, v)
        u2, v2, err2 = evaluator._sinkhorn_potentials(St, BETA, log_mu, log_nu, n_iter, 1)
        assert _same_bits(u2.cpu().numpy(), u.cpu().numpy()) and _same_bits(v2.cpu().numpy(), v.cpu().numpy()) and err2 == err
        tag = f"({n},{L}) it={n_iter}"
        _within(f"{tag} u", u.cpu().numpy(), u32, u64)
        _within(f"{tag} v", v.cpu().numpy(), v32, v64)
        _, d32 = _within(f"{tag} T", T.cpu().numpy(), T32, T64)
        # the row error: LSE is 1-Lipschitz in the largest entry error, so T within the bar moves a row's mass by at most
        # exp(bar) - 1 relative; a second bar covers the float32 evaluation of that LSE and of the exp (the same roundings)
        tol = (1 + e64) * np.expm1(2 * SPREAD * d32)
        print(f"{tag} marginal_err: GPU {err:.6e}   fp64 {e64:.6e}   float32 {e32:.6e}   bar {tol:.3e}")
        assert abs(err - e64) <= tol
        errs[n_iter] = err
    assert errs[50] < errs[5] < errs[1]


# ---- 3. the sharded evaluator under emulated ranks ----------------------------------------------------------------------------------
def _emulated(W, fn, max_sweeps):
    world = comm.EmulatedWorld(W, real_collectives=False)
    out = {}

    def run(r):
        c = world.comm(r)
        with comm.use(c):
            c.begin_step()
            out[r] = fn(SimpleNamespace(world_size=W), r)
    world.settle(run, max_sweeps=max_sweeps)
    return [out[r] for r in range(W)]


def _model():
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(), strict=False)
    return m.to(DEV).eval()


def _testset(n=N, seed=4242):
    t, v, tm, vm = synth.make_samples(seed, "test", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, v, tm.astype(np.float32), vm.astype(np.float32)))


def _bank(n=40, seed=77):
    """The bank of test_hubnorm_gpu.py."""
    t, v, tm, vm = synth.make_samples(seed, "train", n, Nt, Nv)
    return tuple(torch.from_numpy(a).to(DEV) for a in (t, tm.astype(np.float32), v, vm.astype(np.float32)))


def _full(m, a, b, am, bm):
    return evaluator._slab_similarity(m, a, b, am, bm, 0, a.shape[0]).cpu().numpy()


def _margin_ok(M, tol=1e-4):
    """No rank-deciding pair (a query's own score against another) within a relative tol."""
    M = np.asarray(M, dtype=np.float64)
    d = np.diag(M)[:, None]
    gap = np.abs(M - d) / np.maximum(np.maximum(np.abs(M), np.abs(d)), 1e-30)
    np.fill_diagonal(gap, np.inf)
    return bool(gap.min() > tol)


def _lists_ok(M, k, tol=1e-4):
    """No top-k list of a row of M whose k-th and (k+1)-th entries lie within a relative tol (list membership is decided)."""
    top = -np.sort(-np.asarray(M, dtype=np.float64), axis=1)[:, :k + 1]
    return bool(np.all((top[:, k - 1] - top[:, k]) / np.maximum(np.abs(top[:, k - 1]), 1e-30) > tol))


HK = 5                                                       # hubness_k of the evaluator tests


def _restated(mode, S, n_iter, bank_sims=None):
    """(T, V) of the fp64 restatement (sinkhorn: V is T)."""
    if mode == "sinkhorn":
        T = K.sinkhorn(S, BETA, n_iter)[0]
        return T, T
    Qt, Qv = bank_sims
    v_t = K.potentials(Qt, BETA, n_iter)[1]
    u_v = K.potentials(Qv, BETA, n_iter)[0]
    A = K.beta_s(S, BETA)
    return A + v_t[None, :], A + u_v[:, None]


_SETS = {}


def _separated_set(m, mode, n_iter, bank, n=48):
    """(seed, testset, T64, V64): the first seeded set whose fp64 restatement is well separated -- it alone decides."""
    if (mode, n_iter, n) not in _SETS:
        _SETS[(mode, n_iter, n)] = _find_separated_set(m, mode, n_iter, bank, n)
    return _SETS[(mode, n_iter, n)]


def _find_separated_set(m, mode, n_iter, bank, n):
    for seed in range(100, 180):
        t, v, tm, vm = _testset(n, seed)
        S = _full(m, t, v, tm, vm)
        sims = None
        if mode == "qbsinkhorn":
            sims = (_full(m, bank[0], v, bank[1], vm), _full(m, t, bank[2], tm, bank[3]))
        T, V = _restated(mode, S, n_iter, sims)
        if _margin_ok(T) and _margin_ok(V.T) and _lists_ok(T, HK) and _lists_ok(V.T, HK):
            return seed, (t, v, tm, vm), T, V
    raise AssertionError("no well-separated seeded set found")


def _same_metrics(a, b, skip=()):
    assert set(a) == set(b)
    for key in a:
        if key in skip:
            continue
        if key == "hubness":
            for hk in a[key]:
                if isinstance(a[key][hk], np.ndarray):
                    assert np.array_equal(a[key][hk], b[key][hk]), hk
                else:
                    assert a[key][hk] == b[key][hk], hk
        else:
            assert a[key] == b[key], key


def _check_against_restatement(t2v, v2t, T64, V64, mode, n_iter):
    rt, rv = K.single_ranks(T64), K.single_ranks(V64.T)
    assert t2v["cols"] == rt.tolist() and v2t["cols"] == rv.tolist()
    for k in (1, 5, 10):
        assert t2v[f"R{k}"] == K.recall(rt, k) and v2t[f"R{k}"] == K.recall(rv, k), k
    assert np.array_equal(t2v["hubness"]["occurrence"], H.hubness(T64, HK)[0]["occ"])
    assert np.array_equal(v2t["hubness"]["occurrence"], H.hubness(V64, HK)[1]["occ"])
    for d in (t2v, v2t):
        assert d["mode"] == mode and d["beta"] == BETA and d["iters"] == n_iter and 0 <= d["marginal_err"] < np.inf
        assert "qb_k" not in d


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_evaluator_under_emulated_ranks_equals_the_restatement(mode, W):
    n_iter = 6                                               # the emulated world settles one dependent collective per sweep
    m = _model()
    bank = _bank() if mode == "qbsinkhorn" else None
    _, (t, v, tm, vm), T64, V64 = _separated_set(m, mode, n_iter, bank)
    sweeps = 2 * (n_iter + 1) + 16                           # both bank products' iterations, then the metrics' collectives

    def fn(a, r):
        return evaluator.sharded_normalised_metrics(m, t, v, tm, vm, a, mode, BETA, querybank=bank, hubness_k=HK, n_iter=n_iter)
    outs = _emulated(W, fn, sweeps)
    for met in outs:
        _same_metrics(met[0], outs[0][0])
        _same_metrics(met[1], outs[0][1])
    _check_against_restatement(outs[0][0], outs[0][1], T64, V64, mode, n_iter)
    if mode == "sinkhorn":
        assert outs[0][0]["marginal_err"] == outs[0][1]["marginal_err"]

    # the slabs: one output for sinkhorn; values within the measured bar of the restatement
    def slabs(a, r):
        T, V = evaluator.sharded_normalised_slabs(m, t, v, tm, vm, a, mode, BETA, querybank=bank, n_iter=n_iter)
        assert (V is T) == (mode == "sinkhorn")
        return T.cpu().numpy(), V.cpu().numpy()
    parts = _emulated(W, slabs, sweeps)
    T = np.concatenate([p[0] for p in parts])
    V = np.concatenate([p[1] for p in parts])
    S = _full(m, t, v, tm, vm)
    if mode == "sinkhorn":
        _within(f"W={W} T", T, K.sinkhorn(S, BETA, n_iter, dtype=np.float32)[0], T64)
    else:
        Qt, Qv = _full(m, bank[0], v, bank[1], vm), _full(m, t, bank[2], tm, bank[3])
        T32, V32, _, _ = K.qbsinkhorn(S, Qt, Qv, BETA, n_iter, dtype=np.float32)
        _within(f"W={W} T", T, T32, T64)
        _within(f"W={W} V", V, V32, V64)


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_every_rank_holds_the_same_potentials(W):
    n_iter, n, L = 6, 101, 67
    S = _hub_matrix(n, L, 31 + W)
    S[5, 9], S[40, :] = np.nan, np.nan
    St = _dev(S)
    log_mu, log_nu = evaluator._log_marginals(n, L, None, DEV)

    def fn(a, r):
        r0, r1 = evaluator.slab_bounds(n, W, r)
        u, v, err = evaluator._sinkhorn_potentials(St[r0:r1].contiguous(), BETA, log_mu[r0:r1].contiguous(), log_nu, n_iter, W)
        return u.cpu().numpy(), v.cpu().numpy(), err
    outs = _emulated(W, fn, n_iter + 8)
    for o in outs:
        assert _same_bits(o[1], outs[0][1]) and o[2] == outs[0][2]          # v and the error: the same bits on every rank
    u = np.concatenate([o[0] for o in outs])
    T64, u64, v64, e64 = K.sinkhorn(S, BETA, n_iter)
    T32, u32, v32, _ = K.sinkhorn(S, BETA, n_iter, dtype=np.float32)
    assert u[40] == 0
    _within(f"W={W} u", u, u32, u64)
    _within(f"W={W} v", outs[0][1], v32, v64)
    # against one rank: the ranks' column combine associates differently, last bits only (both lie within the bar of fp64)
    if W > 1:
        one = evaluator._sinkhorn_potentials(St, BETA, log_mu, log_nu, n_iter, 1)[1].cpu().numpy()
        assert np.abs(outs[0][1].astype(np.float64) - one).max() <= 2 * SPREAD * _dist(v32, v64)


def test_qbsinkhorn_slabs_are_the_is_apply_with_the_gpus_own_potentials():
    m = _model()
    t, v, tm, vm = _testset()
    bank = _bank()
    n_iter = 50
    args = SimpleNamespace(world_size=1)
    T, V = evaluator.sharded_normalised_slabs(m, t, v, tm, vm, args, "qbsinkhorn", BETA, querybank=bank, n_iter=n_iter)
    Qt, Qv = evaluator._bank_slabs(m, t, v, tm, vm, bank, 1, 0)
    mu_t, nu_t = evaluator._log_marginals(Qt.shape[0], Qt.shape[1], None, DEV)
    mu_v, nu_v = evaluator._log_marginals(Qv.shape[0], Qv.shape[1], None, DEV)
    _, v_t, _ = evaluator._sinkhorn_potentials(Qt, BETA, mu_t, nu_t, n_iter, 1)
    u_v, _, _ = evaluator._sinkhorn_potentials(Qv, BETA, mu_v, nu_v, n_iter, 1)
    S = _full(m, t, v, tm, vm)
    assert _same_bits(T.cpu().numpy(), R.is_scores(S, BETA, -v_t.cpu().numpy(), 0))
    assert _same_bits(V.cpu().numpy(), R.is_scores(S, BETA, -u_v.cpu().numpy(), 1))
    # and those potentials are the restatement's, within the measured bar
    Qt, Qv = Qt.cpu().numpy(), Qv.cpu().numpy()
    _within("v_t", v_t.cpu().numpy(), K.potentials(Qt, BETA, n_iter, dtype=np.float32)[1], K.potentials(Qt, BETA, n_iter)[1])
    _within("u_v", u_v.cpu().numpy(), K.potentials(Qv, BETA, n_iter, dtype=np.float32)[0], K.potentials(Qv, BETA, n_iter)[0])


@pytest.mark.parametrize("mode", MODES)
def test_multi_sentence_fixture_under_emulated_ranks(mode):
    g = golden("multi_sentence")
    S, cut = g["S"].astype(np.float32), g["cut_off_points"].tolist()
    Ns, V_ = S.shape
    ends = np.asarray(cut, dtype=np.int64) + 1
    St = _dev(S)
    n_iter, M = 6, 9
    rng = np.random.default_rng(3)
    Qt_np = rng.uniform(-1, 1, (M, V_)).astype(np.float32)
    Qv_np = rng.uniform(-1, 1, (Ns, 11)).astype(np.float32)
    Qt_full, Qv_full = _dev(Qt_np), _dev(Qv_np)
    if mode == "sinkhorn":                                   # the group-size marginals
        T64 = K.sinkhorn(S, BETA, n_iter, cut)[0]
        T32 = K.sinkhorn(S, BETA, n_iter, cut, dtype=np.float32)[0]
        V64, V32 = T64, T32
        sizes = np.diff(np.concatenate(([0], ends)))
        assert len(set(sizes.tolist())) > 1                  # unequal groups: not the uniform marginals
    else:
        T32, V32, _, _ = K.qbsinkhorn(S, Qt_np, Qv_np, BETA, n_iter, dtype=np.float32)
        T64, V64 = _restated(mode, S, n_iter, (Qt_np, Qv_np))
    for W in (1, 2, 3):
        def fn(a, r, W=W):
            r0, r1 = evaluator.slab_bounds(Ns, W, r)
            q0, q1 = evaluator.slab_bounds(M, W, r)
            bank = (Qt_full[q0:q1].contiguous(), Qv_full[r0:r1].contiguous()) if mode == "qbsinkhorn" else None
            T, V, info = evaluator._sinkhorn_from_slab(St[r0:r1].contiguous(), Ns, V_, W, r, mode, BETA, n_iter, ends, bank, M)
            met = evaluator._metrics_from_normalised(T, V, Ns, V_, W, r, ends, 3)
            return T.cpu().numpy(), V.cpu().numpy(), met, info
        outs = _emulated(W, fn, 2 * (n_iter + 1) + 16)
        T = np.concatenate([o[0] for o in outs])
        Vn = np.concatenate([o[1] for o in outs])
        for o in outs:
            _same_metrics(o[2][0], outs[0][2][0])
            _same_metrics(o[2][1], outs[0][2][1])
            assert o[3] == outs[0][3] and o[3]["iters"] == n_iter
        t2v, v2t = outs[0][2]
        # the metrics are those of the rank rules on the GPU's T; T itself against the restatement
        rt, rv = K.group_ranks(T, cut), K.single_ranks(K.group_max(Vn, cut))
        want_t = training.RetrievalMetrics.multi_sentence_metrics_from_ranks(rt)
        want_v = training.RetrievalMetrics.metrics_from_ranks(rv)
        for key in ("R1", "R5", "R10", "MedianR", "MeanR"):
            assert t2v[key] == want_t[key] and v2t[key] == want_v[key], (W, key)
        ht, hv = H.hubness(T, 3, cut)[0], H.hubness(Vn, 3, cut)[1]
        assert np.array_equal(t2v["hubness"]["occurrence"], ht["occ"]) and np.array_equal(v2t["hubness"]["occurrence"], hv["occ"])
        _within(f"{mode} W={W} T", T, T32, T64)
        _within(f"{mode} W={W} V", Vn, V32, V64)


# ---- 4. two gloo ranks, one child process each --------------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, seed, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    torch.manual_seed(20240607)
    args = SimpleNamespace(world_size=world, local_rank=rank)
    m = _model()
    res = {}
    for mode in MODES:
        t, v, tm, vm = _testset(48, seed[mode])
        res[mode] = evaluator.sharded_normalised_metrics(m, t, v, tm, vm, args, mode, BETA, querybank=_bank(), hubness_k=HK)
    torch.save(res, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_a_single_process(tmp_path):
    m = _model()
    bank = _bank()
    n_iter = 50                                              # the default
    sets = {mode: _separated_set(m, mode, n_iter, bank) for mode in MODES}
    world, port = 2, 29683
    out = str(tmp_path / "res")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    seeds = ",".join(f"{mode}={sets[mode][0]}" for mode in MODES)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--gloo-worker", str(r), str(world), str(port), seeds, out],
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
    args1 = SimpleNamespace(world_size=1)
    for mode in MODES:
        _, (t, v, tm, vm), T64, V64 = sets[mode]
        one = evaluator.sharded_normalised_metrics(m, t, v, tm, vm, args1, mode, BETA, querybank=bank, hubness_k=HK)
        assert one[0]["iters"] == n_iter
        _check_against_restatement(one[0], one[1], T64, V64, mode, n_iter)
        for r in range(world):
            res = torch.load(f"{out}.{r}", weights_only=False)[mode]
            for d in range(2):
                # the same metrics; the ranks' column combine associates differently from one rank's, so T may differ in
                # its last bits (ulp(32) = 3.8e-6) and with it a row's mass
                _same_metrics(res[d], one[d], skip=("marginal_err",))
                assert abs(res[d]["marginal_err"] - one[d]["marginal_err"]) <= 1e-5


# ---- 5. eval_epoch and main_retrieval.py -----------------------------------------------------------------------------------------------
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
    return SimpleNamespace(world_size=1, rank=0, local_rank=0, logger=logging.getLogger("test_sinknorm"), **over)


def _strip(d):
    return {k: v for k, v in d.items() if k not in ("test_norm", "hubness")}


def _bank_model(bank):
    m = _model()
    m.mb_ind = torch.arange(bank[0].shape[0], device=DEV)
    m.mb_feat_t, m.mb_mask_t, m.mb_feat_v, m.mb_mask_v = bank
    return m


EVAL_BETA = 100.0      # the synthetic similarities span 0 .. 0.12, so at beta = 20 the rows are balanced to the float32 floor
#                        of the row error (about 1e-6: a few ulp of the mass 1) after 3 iterations, and 5 and 50 iterations report
#                        the same figure; at beta = 100 the oracle's similarity gives about 2e-3 after 5 and the floor after 20


def test_eval_epoch_single_sentence_with_each_mode(caplog):
    t, v, tm, vm = (x.cpu() for x in _testset())
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    loader = Loader(_batches(t, v, tm, vm, order, 32))
    bank = _bank()
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="test_sinknorm"):
        base = training.eval_epoch(_args(), _model(), loader, torch.device(DEV))
    plain = [r.getMessage() for r in caplog.records if "Feature extraction" not in r.getMessage() and "Similarity + metrics" not in r.getMessage()]
    for mode in MODES:
        errs = {}
        for n_iter in (5, 50):
            caplog.clear()
            with caplog.at_level(logging.INFO, logger="test_sinknorm"):
                on = training.eval_epoch(_args(test_norm=mode, test_norm_beta=EVAL_BETA, test_norm_iters=n_iter, hubness_k=5),
                                         _bank_model(bank), loader, torch.device(DEV))
            lines = [r.getMessage() for r in caplog.records]
            tag = evaluator.test_norm_label(mode, EVAL_BETA, n_iter)
            assert tag == f"[{evaluator.TEST_NORM_LABELS[mode]} b=100 it={n_iter}]"
            assert any(line.startswith(f"Text-to-Video {tag}: R@1") for line in lines), lines
            assert any(line.startswith(f"Video-to-Text {tag}: R@1") for line in lines)
            assert sum(f"{tag} Hubness@5" in line for line in lines) == 2
            assert sum(line.startswith(f"{tag} marginal error") for line in lines) == 1
            # every other line is the plain run's (but its raw hubness lines and the two timings)
            rest = [line for line in lines if tag not in line and "Hubness@5" not in line and "Feature extraction" not in line
                    and "Similarity + metrics" not in line]
            assert rest == plain
            assert _strip(on[0]) == base[0] and _strip(on[1]) == base[1]
            want = evaluator.sharded_normalised_metrics(_model(), t.to(DEV), v.to(DEV), tm.to(DEV), vm.to(DEV), _args(), mode, EVAL_BETA,
                                                        querybank=bank, hubness_k=5, n_iter=n_iter)
            _same_metrics(on[0]["test_norm"], want[0])
            _same_metrics(on[1]["test_norm"], want[1])
            assert on[0]["test_norm"]["iters"] == n_iter
            errs[n_iter] = (on[0]["test_norm"]["marginal_err"], on[1]["test_norm"]["marginal_err"])
        assert errs[50][0] < errs[5][0] and errs[50][1] < errs[5][1], errs
    # the default is the reference's 50 iterations
    on = training.eval_epoch(_args(test_norm="sinkhorn"), _model(), loader, torch.device(DEV))
    assert on[0]["test_norm"]["iters"] == 50
    with pytest.raises(ValueError, match="load_memory_bank"):
        training.eval_epoch(_args(test_norm="qbsinkhorn"), _model(), loader, torch.device(DEV))
    with pytest.raises(ValueError):
        training.eval_epoch(_args(test_norm="sinkhorn", test_norm_iters=0), _model(), loader, torch.device(DEV))


def test_eval_epoch_multi_sentence_with_sinkhorn():
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
    base = training.eval_epoch(_args(), _model(), loader, torch.device(DEV))
    on = training.eval_epoch(_args(test_norm="sinkhorn", test_norm_iters=20), _model(), loader, torch.device(DEV))
    assert _strip(on[0]) == base[0] and _strip(on[1]) == base[1]
    want = evaluator.sharded_normalised_metrics(_model(), t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float(), _args(),
                                                "sinkhorn", BETA, cut_off_points=(ends - 1).tolist(), n_iter=20)
    _same_metrics(on[0]["test_norm"], want[0])
    _same_metrics(on[1]["test_norm"], want[1])
    # the group-size marginals, not the uniform ones: the slab against the restatement
    m = _model()
    T, V = evaluator.sharded_normalised_slabs(m, t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float(), _args(), "sinkhorn", BETA,
                                              cut_off_points=(ends - 1).tolist(), n_iter=20)
    assert V is T
    S = _full(m, t.to(DEV), v.to(DEV), tm.to(DEV).float(), vm.to(DEV).float())
    cut = (ends - 1).tolist()
    _within("multi-sentence T", T.cpu().numpy(), K.sinkhorn(S, BETA, 20, cut, dtype=np.float32)[0], K.sinkhorn(S, BETA, 20, cut)[0])


def test_main_retrieval_logs_sinkhorn_metrics_only_with_the_flag():
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--synthetic_test", "200"]
    outs = []
    for extra in ([], ["--test_norm", "sinkhorn"], ["--test_norm", "qbsinkhorn", "--hubness_k", "15", "--test_norm_iters", "5"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([line.split(" ", 1)[1] for line in r.stdout.splitlines() if line.strip()])
    plain, sk, qb = outs
    assert not any("Sinkhorn" in line for line in plain)
    extra_sk = [line for line in sk if "[Sinkhorn b=20 it=50]" in line]
    assert len(extra_sk) == 2 and extra_sk[0].startswith("text->video [Sinkhorn b=20 it=50] R@1")
    assert extra_sk[1].startswith("[Sinkhorn b=20 it=50] marginal error")
    assert [line for line in sk if "[Sinkhorn" not in line] == plain
    extra_qb = [line for line in qb if "[QB-Sinkhorn b=20 it=5]" in line]
    assert len(extra_qb) == 4 and sum("Hubness@15" in line for line in extra_qb) == 2
    raw_qb = [line for line in qb if "[QB-Sinkhorn" not in line and "Hubness@" not in line and "memory bank" not in line]
    assert raw_qb == plain


if __name__ == "__main__":                                   # one gloo rank of test_two_gloo_ranks_equal_a_single_process
    if len(sys.argv) == 7 and sys.argv[1] == "--gloo-worker":
        seeds = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in sys.argv[5].split(",")}
        _gloo_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), seeds, sys.argv[6])
