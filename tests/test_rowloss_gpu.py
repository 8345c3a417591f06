"""GPU: every launch form of the row-loss tail (csrc/nr_rowloss.hip, the uniform rows of csrc/nr_sinkhorn.hip, nr_loss_finalize,
nr_rowloss_coef, nr_rowloss_bwd_finish) against the per-row fp64 reference of tests/rowloss_ref.py.

Every comparison is per row and per term, on ALL rows of both directions: max|kernel - fp64| over the rows of a term, relative
to max|fp64| of that term in the case.  The bars are rowloss_ref.BAR_FWD / BAR_BWD: 8 x the error of the same formulas in plain
fp32 on the CPU on exactly these inputs (measured and re-asserted by tests/test_rowloss_cpu.py, never taken from a kernel);
the uniform rows of the Sinkhorn kernel (fast exp / log / rcp and the matrix-scaling iteration) keep the suite's 2e-5.  A NaN
on either side fails, except in the neighbour rows of the two cases whose REFERENCE is NaN there (one sample outside the
neighbour set; a constant c): their NaN positions must be the reference's.

  (a) the plain forward at every NE instance and both sides of every valid[] switch, edges of K, planted ties, constant c
  (b) the forms that must equal (a) bit for bit: self-finalizing, without the uniform term, slab
  (c) nr_loss_finalize against the arithmetic of nr_finalize.h in fp64
  (d) bank centralities from partial sums, paired with the Sinkhorn launch as head.py runs them, both launch orders
  (e) centrality weights computed by the row's own wave
  (f) the uniform term from the Sinkhorn kernel
  (g) the backward: coefficient launch -> row kernel -> finish launch, all seven gradients; the slab form bit for bit"""
import functools
from types import SimpleNamespace

import pytest
import torch

import nr_oracle as O
import rowloss_ref as R
from neighborretr_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
INPUTS = ("S", "G", "tgt_rows", "tgt_cols", "c0", "c1", "w_t", "w_v", "ls")


def _to_dev(q):
    g = SimpleNamespace(B=q.B, K=q.K, T=q.T)
    for name in INPUTS:
        setattr(g, name, getattr(q, name).to(DEV).contiguous())
    return g


def _args(g):
    return tuple(getattr(g, name) for name in INPUTS)


@functools.lru_cache(maxsize=4)
def _case(seed, B, K, opt=""):
    """(inputs on the CPU, the same on the device, fp64 rows [2, 4, B]) -- computed once, shared, never written to."""
    q = R.make_case(seed, B, K, ties=opt == "ties", const_c=opt == "const_c")
    return q, _to_dev(q), R.case_terms(q)


def _check_rows(tag, got, ref, bars, terms=(0, 1, 2, 3), nan_neighbour=False):
    """Per term: every row of both directions within bars[term] * max|ref term|.  Prints every figure, then asserts."""
    got = got.detach().cpu().double()
    bad = []
    for k in terms:
        name = R.TERMS[k]
        if k == 2 and nan_neighbour:
            same = torch.equal(torch.isnan(got[:, 2]), torch.isnan(ref[:, 2]))
            print(f"rowloss {tag}: neighbour NaN positions {'equal' if same else 'DIFFER'} ({int(torch.isnan(ref[:, 2]).sum())} NaN rows)")
            if not same or not bool(torch.isnan(ref[:, 2]).any()):
                bad.append(name)
            continue
        assert bool(torch.isfinite(ref[:, k]).all()), (tag, name, "the reference is not finite")
        r = R.rel_err(got[:, k], ref[:, k])
        print(f"rowloss {tag}: {name} {r:.2e} of max|ref| {float(ref[:, k].abs().max()):.3g} (bar {bars[name]:.1e})")
        if not r <= bars[name]:                                      # NaN fails
            bad.append(f"{name} {r:.2e} > {bars[name]:.1e}")
    assert not bad, (tag, bad)


def _loss_bounds(ref, bars, wu, wn, wkl):
    """Absolute bounds for the five losses given per-row bounds: a mean of rows errs by at most the largest row error, plus
    2e-6 of the mean magnitude for the fp32 reduction of nr_finalize.h (17 serial adds + 6 tree levels + 4 operations at 2^-24)."""
    B = ref.shape[-1]
    b = [bars[R.TERMS[k]] * float(ref[:, k].abs().max()) + 2e-6 * float(ref[:, k].abs().mean()) for k in range(4)]
    b[3] /= B
    return [b[0] + wu * b[1] + wn * b[2] + wkl * b[3]] + b


def _check_losses(tag, losses, ref_rows, bars, wts):
    want = R.five_losses(ref_rows, *wts)
    bound = _loss_bounds(ref_rows, bars, *wts)
    diff = (losses.detach().cpu().double() - want).abs().tolist()
    print(f"losses {tag}: |d| " + " ".join(f"{d:.2e}/{b:.1e}" for d, b in zip(diff, bound)))
    assert all(d <= b for d, b in zip(diff, bound)), (tag, diff, bound)


# ---- (a) the plain forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,opt", R.FWD_CASES, ids=[f"{B}-{K}{'-' + o if o else ''}" for B, K, o in R.FWD_CASES])
def test_plain_forward_against_fp64_rows(B, K, opt):
    q, g, ref = _case(R.SEED_FWD, B, K, opt)
    rows = ops.row_losses(*_args(g), K, q.T)
    _check_rows(f"plain B={B} K={K} {opt}", rows, ref, R.BAR_FWD, nan_neighbour=opt in ("nan", "const_c"))
    if K == 0:
        assert float(rows[:, 2].abs().max()) == 0.0


def test_plain_forward_refuses_what_it_does_not_cover():
    z = torch.zeros(2049, 2049, device=DEV)
    v = torch.zeros(2049, device=DEV)
    with pytest.raises(hip.NrHipError):                                  # B > 2048: no NE instance
        ops.row_losses(z, z, z, z, v, v, v, v, torch.ones(1, device=DEV), 20, 3.0)
    q, g, _ = _case(R.SEED_FWD, 13, 13)
    with pytest.raises(hip.NrHipError):                                  # K = B + 1: the reference raises IndexError
        ops.row_losses(*_args(g), 14, q.T)


# ---- (b) forms that equal (a) bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(5, 2), (129, 20), (1025, 20)])
def test_self_finalizing_form_is_the_plain_form_and_loss_finalize(B, K):
    q, g, _ = _case(R.SEED_FWD, B, K)
    rows = ops.row_losses(*_args(g), K, q.T)
    want = ops.loss_finalize(rows, 1.0, 0.5, 2.0)
    for _ in range(3):                                                   # the counter resets itself
        rows2, losses = ops.row_losses_final(*_args(g), K, q.T, 1.0, 0.5, 2.0)
        assert torch.equal(rows, rows2) and torch.equal(want, losses)


@pytest.mark.parametrize("B,K", [(5, 2), (65, 20), (129, 20), (257, 20)])
def test_form_without_the_uniform_term_leaves_it_alone(B, K):
    q, g, _ = _case(R.SEED_FWD, B, K)
    rows = ops.row_losses(*_args(g), K, q.T)
    rl = torch.full((2, 4, B), -777.0, device=DEV)
    ops.row_losses_no_uniform(g.S, g.G, g.c0, g.c1, g.w_t, g.w_v, g.ls, K, q.T, rl)
    assert torch.equal(rl[:, [0, 2, 3]], rows[:, [0, 2, 3]])
    assert bool((rl[:, 1] == -777.0).all())


def _slabs(g, row0, n):
    return g.S[row0:row0 + n].contiguous(), g.S[:, row0:row0 + n].contiguous()


@pytest.mark.parametrize("B,row0,n", R.SLABS)
def test_slab_form_equals_the_plain_rows(B, row0, n):
    q, g, ref = _case(R.SEED_FWD, B, 20)
    rows = ops.row_losses(*_args(g), 20, q.T)
    _check_rows(f"plain B={B} K=20", rows, ref, R.BAR_FWD)
    S_rows, S_cols = _slabs(g, row0, n)
    slab = ops.row_losses_slab(S_rows, S_cols, row0, *_args(g)[1:], 20, q.T)
    assert torch.equal(slab[:, :, row0:row0 + n], rows[:, :, row0:row0 + n])
    outside = torch.ones(B, dtype=torch.bool, device=DEV)
    outside[row0:row0 + n] = False
    assert bool((slab[:, :, outside] == 0.0).all())                      # rows outside the slab are still zero


# ---- (c) the five losses ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(3, 2), (65, 20), (1025, 20)])
def test_loss_finalize_against_fp64(B, K):
    q, g, _ = _case(R.SEED_FWD, B, K)
    rows = ops.row_losses(*_args(g), K, q.T)
    assert bool(torch.isfinite(rows).all())
    losses = ops.loss_finalize(rows, 1.0, 0.5, 2.0)
    zero = {t: 0.0 for t in R.TERMS}                                     # the kernel's own rows: only the reduction is at stake
    _check_losses(f"finalize B={B}", losses, rows.cpu().double(), zero, (1.0, 0.5, 2.0))


# ---- the pair of the loss-only step: Sinkhorn launch + row-loss launch sharing one counter ----------------------------------
def _pair(g, G, beta, iters, row_launch, sinkhorn_first, wts):
    """rowloss [2, 4, B] (NaN-filled first) and the five losses from the two self-finalizing launches, in either order."""
    rl = torch.full((2, 4, g.B), float("nan"), device=DEV)
    losses = torch.full((5,), float("nan"), device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    sk = lambda: ops.sinkhorn_uniform_rows_final(G, beta, g.T, rl, counter, *wts, losses, iters)
    row = lambda: row_launch(rl, counter, losses)
    for launch in ((sk, row) if sinkhorn_first else (row, sk)):
        launch()
    torch.cuda.synchronize()
    assert int(counter) == 0
    return rl, losses


@functools.lru_cache(maxsize=None)
def _plans(seed, B, iters, sigma=6.0, diag=8.0):
    """G and the fp64 transport plans Q of G and of G.t() after `iters` iterations (targets = beta Q + (1 - beta) I)."""
    G = R.make_G(seed, B, sigma, diag)
    return G, O.sinkhorn_targets(G.double(), 1.0, iters), O.sinkhorn_targets(G.double().t(), 1.0, iters)


def _uniform_ref(seed, B, beta, iters, T, sigma=6.0, diag=8.0):
    G, Qr, Qc = _plans(seed, B, iters, sigma, diag)
    eye = torch.eye(B, dtype=torch.float64)
    return R.uniform_rows(G, beta * Qr + (1 - beta) * eye, beta * Qc + (1 - beta) * eye, T)


# ---- (d) bank centralities from partial sums --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", R.PARTS_B)
def test_partial_sums_with_the_sinkhorn_half_both_orders(B, K):
    q, g, _ = _case(R.SEED_PARTS, B, K)
    wts = (1.0, 0.7, 1.3)
    uni = R.uniform_rows(q.G, O.sinkhorn_targets(q.G.double(), 0.7, 50), O.sinkhorn_targets(q.G.double().t(), 0.7, 50), q.T)
    bars = dict(R.BAR_FWD, uniform=R.BAR_SINKHORN_UNIFORM)
    for n0, n1 in R.PARTS_N:
        for sc in R.PARTS_SCALE:
            p0, p1 = R.make_parts(R.SEED_PARTS, B, n0, sc, "c0"), R.make_parts(R.SEED_PARTS, B, n1, sc, "c1")
            ref = R.case_terms(q, c0=R.centres_from_parts(p0, sc), c1=R.centres_from_parts(p1, sc))
            ref[:, 1] = uni
            p0, p1 = p0.to(DEV), p1.to(DEV)
            launch = lambda rl, counter, losses: ops.row_losses_no_uniform_final(
                g.S, g.G, p0, p1, sc, g.w_t, g.w_v, g.ls, K, q.T, rl, counter, *wts, losses)
            out = [_pair(g, g.G, 0.7, 50, launch, first, wts) for first in (True, False)]
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
            tag = f"parts B={B} n=({n0},{n1}) scale=1/{round(1 / sc)}"
            _check_rows(tag, out[0][0], ref, bars)
            _check_losses(tag, out[0][1], ref, bars, wts)


# ---- (e) centrality weights computed in the row's wave ----------------------------------------------------------------------
@pytest.mark.parametrize("d", R.CW_D)
@pytest.mark.parametrize("B,K", R.CW_B)
def test_centrality_weights_inside_the_row_launch(B, K, d):
    q, g, _ = _case(R.SEED_CW, B, K)
    wts = (1.0, 0.7, 1.3)
    sc = 1.0 / 512
    gt, gv, mt, mv = R.make_cw(R.SEED_CW, B, d)
    p0, p1 = R.make_parts(R.SEED_CW, B, 3, sc, "c0"), R.make_parts(R.SEED_CW, B, 4, sc, "c1")
    ref = R.case_terms(q, c0=R.centres_from_parts(p0, sc), c1=R.centres_from_parts(p1, sc),
                       w_t=R.centrality_weights(gt, mt, R.CW_SCALE), w_v=R.centrality_weights(gv, mv, R.CW_SCALE))
    gt, gv, mt, mv, p0, p1 = (t.to(DEV) for t in (gt, gv, mt, mv, p0, p1))
    launch = lambda rl, counter, losses: ops.row_losses_no_uniform_final_cw(
        g.S, g.G, p0, p1, sc, gt, gv, mt, mv, R.CW_SCALE, g.ls, K, q.T, rl, counter, *wts, losses)
    rl, losses = _pair(g, g.G, 0.7, 50, launch, True, wts)
    _check_rows(f"cw B={B} d={d}", rl, ref, R.BAR_FWD, terms=(0, 2, 3))
    assert bool(torch.isfinite(rl).all()) and bool(torch.isfinite(losses).all())
    # the all-zero row of g: weight EXACTLY 1 -- the same launch with finished weights of 1 gives the same bits in that row
    one = torch.ones(B, device=DEV)
    launch1 = lambda rl, counter, losses: ops.row_losses_no_uniform_final(
        g.S, g.G, p0, p1, sc, one, one, g.ls, K, q.T, rl, counter, *wts, losses)
    rl1, _ = _pair(g, g.G, 0.7, 50, launch1, True, wts)
    assert torch.equal(rl[:, 0, 1], rl1[:, 0, 1])
    assert torch.equal(rl[:, [2, 3]], rl1[:, [2, 3]])                    # the weights touch the centrality term alone


# ---- (f) the uniform term from the Sinkhorn kernel -------------------------------------------------------------------------
def _sinkhorn_uniform(g, G, beta, iters):
    """Term 1 from nr_sinkhorn_uniform_rows (nothing else written) and from nr_sinkhorn_uniform_rows_final (in its pair)."""
    B = g.B
    rl = torch.full((2, 4, B), float("nan"), device=DEV)
    assert ops.sinkhorn_uniform_rows(G, beta, g.T, rl, iters)
    assert bool(torch.isnan(rl[:, [0, 2, 3]]).all())
    wts = (1.0, 0.7, 1.3)
    launch = lambda rl, counter, losses: ops.row_losses_no_uniform_final(
        g.S, G, g.c0[None], g.c1[None], 1.0, g.w_t, g.w_v, g.ls, g.K, g.T, rl, counter, *wts, losses)
    rl2, _ = _pair(g, G, beta, iters, launch, True, wts)
    assert torch.equal(rl[:, 1], rl2[:, 1])
    return rl[:, 1]


@pytest.mark.parametrize("B", R.SINKHORN_B)
def test_uniform_rows_of_the_sinkhorn_kernel_against_fp64(B):
    K = 1 if B < 24 else 20
    q, g, _ = _case(R.SEED_SINKHORN, B, K)
    bad = []
    for iters in R.sinkhorn_iters(B):
        for beta in R.SINKHORN_BETA:
            got = _sinkhorn_uniform(g, g.G, beta, iters).cpu().double()
            want = _uniform_ref(R.SEED_SINKHORN, B, beta, iters, q.T)
            assert torch.equal(_plans(R.SEED_SINKHORN, B, iters)[0], q.G)
            r = R.rel_err(got, want)
            print(f"sinkhorn uniform B={B} iters={iters} beta={beta}: {r:.2e} of max|ref| {float(want.abs().max()):.3g}")
            if not r <= R.BAR_SINKHORN_UNIFORM:
                bad.append((iters, beta, r))
    assert not bad, bad


def test_uniform_rows_of_the_sinkhorn_kernel_on_wide_logits():
    """G = 40 randn: T * G spans about +-400, so the maximum subtraction of the log-sum-exp has to hold.  Finite on both sides
    and within the same 2e-5."""
    B = 64
    q, g, _ = _case(R.SEED_SINKHORN, B, 20)
    G = R.make_G(R.SEED_SINKHORN, B, 40.0, 0.0)
    got = _sinkhorn_uniform(g, G.to(DEV), 0.7, 50).cpu().double()
    want = _uniform_ref(R.SEED_SINKHORN, B, 0.7, 50, q.T, 40.0, 0.0)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(got).all())
    r = R.rel_err(got, want)
    print(f"sinkhorn uniform, wide logits B={B}: {r:.2e} of max|ref| {float(want.abs().max()):.3g}")
    assert r <= R.BAR_SINKHORN_UNIFORM


@pytest.mark.parametrize("B", [20, 128])
def test_targets_written_beside_the_uniform_rows_are_the_targets(B):
    G = R.make_G(R.SEED_SINKHORN, B).to(DEV)
    tr, tc = ops.sinkhorn_targets(G, 0.7, 50)
    tr2, tc2 = torch.full_like(G, float("nan")), torch.full_like(G, float("nan"))
    rl = torch.full((2, 4, B), float("nan"), device=DEV)
    ws = torch.empty((hip.sinkhorn_workspace_bytes(B),), dtype=torch.uint8, device=DEV)
    hip.call("nr_sinkhorn_uniform_rows", hip.ptr(G), B, 0.7, 50, 3.0, hip.ptr(rl.view(-1)[B:]), 4 * B, hip.ptr(tr2), hip.ptr(tc2),
             hip.ptr(ws), hip.stream_ptr())
    assert torch.equal(tr, tr2) and torch.equal(tc, tc2)
    rl0 = torch.full((2, 4, B), float("nan"), device=DEV)
    assert ops.sinkhorn_uniform_rows(G, 0.7, 3.0, rl0, 50)
    assert torch.equal(rl[:, 1], rl0[:, 1])


@pytest.mark.parametrize("B", [130, 6])
def test_uniform_rows_refuse_what_the_one_workgroup_solve_does_not_cover(B):
    G = torch.zeros(B, B, device=DEV)
    rl = torch.full((2, 4, B), float("nan"), device=DEV)
    assert ops.sinkhorn_uniform_rows(G, 0.7, 3.0, rl, 50) is False
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    losses = torch.full((5,), float("nan"), device=DEV)
    with pytest.raises(hip.NrHipError):
        ops.sinkhorn_uniform_rows_final(G, 0.7, 3.0, rl, counter, 1.0, 1.0, 1.0, losses, 50)
    torch.cuda.synchronize()
    assert bool(torch.isnan(rl).all()) and bool(torch.isnan(losses).all()) and int(counter) == 0


# ---- (g) the backward -------------------------------------------------------------------------------------------------------
def _coef(g5, wts, B):
    gs = [None if v is None else torch.tensor([v], device=DEV) for v in g5]
    hp = dict(uniform_weight=wts[0], neighbor_weight=wts[1], kl_weight=wts[2])
    return ops.rowloss_coef(gs, hp, B)


@pytest.mark.parametrize("B,K", R.BWD_CASES)
def test_backward_chain_against_fp64_autograd(B, K):
    q, g, _ = _case(R.SEED_BWD, B, K)
    bad = []
    for n, (g5, wts) in enumerate(R.UPSTREAM):
        want_coef = R.coef(g5, *wts, B)
        coef = _coef(g5, wts, B)
        assert coef.shape == (2, 4, B)
        assert torch.equal(coef, coef[:1, :, :1].expand(2, 4, B))        # one value per term, both directions, every row
        r = R.rel_err(coef.cpu(), want_coef)
        print(f"bwd B={B} K={K} upstream {n}: coef {r:.2e}")
        assert r <= R.BAR_COEF
        dS_dir, dG_dir, dC_rows, d_wc, dls_rows = ops.row_losses_bwd(*_args(g), K, q.T, coef)
        dS, dG, d_c0, d_c1, d_ls = ops.rowloss_bwd_finish(dS_dir, dG_dir, dC_rows, dls_rows)
        got = dict(dS=dS, dG=dG, d_c0=d_c0, d_c1=d_c1, d_w_t=d_wc[0], d_w_v=d_wc[1], d_ls=d_ls)
        want = R.grads(q, want_coef)
        for name in R.GRADS:
            assert got[name].shape == want[name].shape, name
            r = R.rel_err(got[name].cpu(), want[name])
            print(f"bwd B={B} K={K} upstream {n}: {name} {r:.2e} of max|ref| {float(want[name].abs().max()):.3g} (bar {R.BAR_BWD[name]:.1e})")
            if not r <= R.BAR_BWD[name]:
                bad.append(f"upstream {n}: {name} {r:.2e} > {R.BAR_BWD[name]:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("B,row0,n", R.SLABS)
def test_slab_backward_equals_the_full_rows(B, row0, n):
    q, g, _ = _case(R.SEED_FWD, B, 20)
    g5, wts = R.UPSTREAM[1]
    coef = _coef(g5, wts, B)
    full = ops.row_losses_bwd(*_args(g), 20, q.T, coef)
    S_rows, S_cols = _slabs(g, row0, n)
    slab = ops.row_losses_bwd_slab(S_rows, S_cols, row0, *_args(g)[1:], 20, q.T, coef)
    for a, b in zip(slab, full):
        assert a.shape[1] == n and torch.equal(a, b[:, row0:row0 + n].contiguous())
